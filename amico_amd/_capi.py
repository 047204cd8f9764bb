"""ctypes binding of the C ABI in include/amico_amd.h (amico_amd/csrc/libamico_amd.so).

There is NO CPU fallback: if the HIP library is missing or no gfx950 GPU is visible every
entry point raises.  Device memory for the ``*_device`` calls is plain pointers (e.g.
``torch.Tensor.data_ptr()``) -- torch is plumbing, never part of the signatures.
"""
import contextlib
import ctypes as C
import os
from collections import namedtuple
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('AMICO_AMD_LIB') or os.path.join(_HERE, 'csrc', 'libamico_amd.so')   # override: A/B builds

AMX_OK, AMX_E_BADARG, AMX_E_HIP, AMX_E_DIR_OOB, AMX_E_OVERFLOW, AMX_E_NODEVICE = 0, -1, -2, -3, -4, -5
F_RMSE, F_NRMSE, F_MODULATED, F_CORRECTED, F_DEBUG_X, F_FW_ISO = 1, 2, 4, 8, 16, 32
# AMX_T_*: the stored dtypes amx_prep_ingest* converts to float32 on the GPU
RAW_DTYPES = {np.dtype(np.uint8): 1, np.dtype(np.int16): 2, np.dtype(np.uint16): 3, np.dtype(np.int32): 4, np.dtype(np.float32): 5,
              np.dtype(np.float64): 6}

# every symbol include/amico_amd.h declares (tests check that the library exports them all)
SYMBOLS = ['amx_version', 'amx_build_id', 'amx_device_count', 'amx_set_call_voxels', 'amx_ctx_create', 'amx_ctx_destroy', 'amx_last_error',
           'amx_lut_upload_noddi', 'amx_lut_upload_freewater', 'amx_lut_upload_sandi', 'amx_lut_destroy',
           'amx_dir_to_lut_idx', 'amx_noddi_fit', 'amx_freewater_fit', 'amx_sandi_fit',
           'amx_noddi_fit_device', 'amx_freewater_fit_device', 'amx_sandi_fit_device', 'amx_sync_status',
           'amx_noddi_fit_device_f32', 'amx_freewater_fit_device_f32', 'amx_sandi_fit_device_f32', 'amx_czb_fit_device_f32',
           'amx_set_debug_x', 'amx_set_fw_iso', 'amx_freewater_corrected_device', 'amx_prep_corrected_device', 'amx_predict_device', 'amx_prep_predicted_device', 'amx_debug_fetch', 'amx_lut_upload_czb', 'amx_czb_fit', 'amx_czb_fit_f32', 'amx_czb_fit_device', 'amx_noddi_fit_f32', 'amx_freewater_fit_f32', 'amx_sandi_fit_f32', 'amx_set_progress',
           'amx_set_profiling', 'amx_last_kernel_ms', 'amx_last_stats', 'amx_last_seed_stats', 'amx_last_host_narrowed', 'amx_last_path', 'amx_host_pool_info', 'amx_selftest',
           'amx_dti_create', 'amx_dti_create_method', 'amx_dti_create_robust', 'amx_dti_last_unconverged', 'amx_dti_last_trips', 'amx_dti_last_robust', 'amx_dti_destroy', 'amx_dti_directions', 'amx_dti_directions_device', 'amx_dti_directions_device_f32',
           'amx_dti_fit', 'amx_dti_fit_device', 'amx_dti_fit_device_f32', 'amx_dti_fit_robust', 'amx_dti_fit_robust_device', 'amx_dti_fit_robust_device_f32', 'amx_prep_gather_device_f32',
           'amx_prep_create', 'amx_prep_destroy', 'amx_prep_gather', 'amx_prep_gather_device',
           'amx_prep_gather_directions_device', 'amx_prep_gather_directions_device_f32', 'amx_prep_route', 'amx_noddi_route', 'amx_small_route', 'amx_prep_last_launch',
           'amx_prep_mean_b0', 'amx_prep_mean_b0_device', 'amx_prep_scatter', 'amx_prep_scatter_device',
           'amx_debias_rows', 'amx_debias_rows_f32', 'amx_debias_rows_device', 'amx_debias_rows_device_f32',
           'amx_prep_set_debias_mask', 'amx_prep_debias', 'amx_prep_debias_device', 'amx_debias_last_unconverged',
           'amx_noise_b0_rows_device', 'amx_noise_b0_rows_device_f32', 'amx_prep_noise_b0_device', 'amx_nanmedian_device',
           'amx_prep_noise_mppca_device', 'amx_mppca_route', 'amx_prep_noise_mppca_denoise_device', 'amx_mppca_denoise_route',
           'amx_prep_unring_device', 'amx_unring_route',
           'amx_prep_sanitize', 'amx_prep_sanitize_device', 'amx_sanitize_device_f32', 'amx_sanitize_device', 'amx_sanitize', 'amx_sanitize_last', 'amx_sanitize_previous',
           'amx_prep_ingest', 'amx_prep_ingest_device',
           'amx_lut_resample', 'amx_lut_rotate_resample', 'amx_lut_route',
           'amx_dict_upload', 'amx_dict_destroy', 'amx_nnls_batched', 'amx_lasso_batched', 'amx_nnls_batched_device', 'amx_lasso_batched_device',
           'amx_dict_set_dense', 'amx_batched_last_dense',
           'amx_bootstrap_resample_device', 'amx_bootstrap_resample_device_f32', 'amx_bootstrap_accumulate_device', 'amx_bootstrap_std_device']

# one row per model fit: what the C entry points amx_<stem>_fit[_f32] / amx_<stem>_fit_device[_f32] differ in.  lib() makes their argtypes
# from it, _fit_host / _fit_device their calls, models.BaseModel._run the results dict.
#   dirs     the call takes DIRs behind y
#   extras   ctypes of the model's own scalars between lambda2 and flags; the wrappers' `extras` tuple starts with their values and may go
#            on with values only the row's own functions read (NODDI's n_maps)
#   outputs  in ABI order: (result name, wrapper keyword that switches it on (None: always), AMX_F_* flag, trailing shape(lut, extras))
#   x_shape  trailing shape of the AMX_F_DEBUG_X coefficients (return_x)
#   check    the model's own argument check, behind those of y and DIRs (or None)
FitRow = namedtuple('FitRow', 'stem dirs extras outputs x_shape check')
Output = namedtuple('Output', 'name key flag shape')


def _check_n_maps(lut, extras):
    if lut.n_maps is not None and extras[0] != lut.n_maps:      # (the library writes what the DICTIONARY says: a short buffer would be overrun)
        raise ValueError(f'the dictionary writes {lut.n_maps} maps per voxel, the model expects {extras[0]} (isExvivo changed?)')


def _outputs(width, *more):
    return (Output('estimates', None, 0, width), Output('rmse', 'rmse', F_RMSE, lambda lut, ex: ()),
            Output('nrmse', 'nrmse', F_NRMSE, lambda lut, ex: ())) + more


def _atoms(lut):
    return (lut.n_atoms,)


FITS = (
    FitRow('noddi', True, (), _outputs(lambda lut, ex: (ex[0],), Output('estimates_mod', 'mod', F_MODULATED, lambda lut, ex: (2,))),
           lambda lut: (3, lut.n_atoms), _check_n_maps),
    FitRow('freewater', True, (C.c_int,), _outputs(lambda lut, ex: (4 if ex[0] else 2,),
                                                   Output('y_corrected', 'corrected', F_CORRECTED, lambda lut, ex: (lut.nS,))), _atoms, None),
    FitRow('sandi', False, (), _outputs(lambda lut, ex: (6,)), _atoms, None),
    FitRow('czb', True, (), _outputs(lambda lut, ex: (3,)), _atoms, None),
)
FIT = {row.stem: row for row in FITS}

_lib = None
c_vp, c_dp, c_fp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float)
c_i16p, c_i32p, c_i64p = C.POINTER(C.c_int16), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
PROGRESS_CB = C.CFUNCTYPE(None, C.c_int64, C.c_int64, c_vp)


def source_id():
    """sha256[:16] of the library's sources as they are in the tree now (same recipe as amico_amd/csrc/Makefile)"""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, 'csrc')
    files = sorted(glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.hpp')), key=os.path.basename)
    files.append(os.path.join(_HERE, '..', 'include', 'amico_amd.h'))
    h = hashlib.sha256()
    for f in files:
        with open(f, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_id():
    """what the loaded library says it was built from: 'amico_amd <version> csrc <hash>'"""
    return lib().amx_build_id().decode()


def build_is_current():
    return build_id().split()[-1] == source_id()


class AmxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def lib():
    """Load libamico_amd.so (fails loudly when the HIP extension has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'amico_amd: HIP library {LIB_PATH} not found -- run `python -c "import '
                           f'__graft_entry__ as g; g.build()"` (or `make -C amico_amd/csrc -j`). '
                           f'There is no CPU fallback.')
    # torch ships its own copy of the ROCm runtime under the same SONAMEs as /opt/rocm's, and the copy that is loaded
    # first serves the whole process; torch only finds its GPUs on its own copy.  Load torch's first when torch is
    # installed, so that device buffers / streams / torch.distributed keep working next to this library.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.amx_build_id.restype = C.c_char_p
    L.amx_ctx_create.argtypes = [C.c_int, C.POINTER(c_vp)]
    L.amx_ctx_destroy.argtypes = [c_vp]
    L.amx_ctx_destroy.restype = None
    L.amx_last_error.argtypes = [c_vp]
    L.amx_last_error.restype = C.c_char_p
    L.amx_lut_upload_noddi.argtypes = [c_vp, c_fp, c_fp, c_dp, c_fp, c_fp, c_i16p, c_i64p, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.POINTER(c_vp)]
    L.amx_lut_upload_freewater.argtypes = [c_vp, c_fp, c_fp, c_i16p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(c_vp)]
    L.amx_lut_upload_sandi.argtypes = [c_vp, c_dp, c_dp, c_dp, c_dp, c_dp, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(c_vp)]
    L.amx_lut_destroy.argtypes = [c_vp]
    L.amx_lut_destroy.restype = None
    L.amx_dir_to_lut_idx.argtypes = [c_vp, c_vp, c_dp, C.c_int64, c_i32p]
    for row in FITS:                # the 16 fit symbols: the host form takes y as float64 | float32 rows, the device form pointers + the stream
        mid = [C.c_int64, C.c_double, C.c_double] + list(row.extras) + [C.c_uint]
        for sfx, yp in (('', c_dp), ('_f32', c_fp)):
            getattr(L, 'amx_%s_fit%s' % (row.stem, sfx)).argtypes = [c_vp, c_vp, yp] + [c_dp] * row.dirs + mid + [c_dp] * len(row.outputs)
            getattr(L, 'amx_%s_fit_device%s' % (row.stem, sfx)).argtypes = [c_vp] * (3 + row.dirs) + mid + [c_vp] * (len(row.outputs) + 1)
    L.amx_sync_status.argtypes = [c_vp, c_vp]
    L.amx_set_debug_x.argtypes = [c_vp, c_vp]
    L.amx_set_fw_iso.argtypes = [c_vp, c_vp]
    L.amx_freewater_corrected_device.argtypes = [c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int64, c_vp, c_vp]      # ctx, lut, y32, y64, x_iso, n, ycorr, stream
    L.amx_prep_corrected_device.argtypes = [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32p, C.c_int, c_vp, c_vp]  # ctx, plan, lut, y32, x_iso, mean_b0, b0_cols (host), n, volume, stream
    L.amx_predict_device.argtypes = [c_vp, c_vp, c_vp, C.c_int64, C.c_int64, c_vp, C.c_int64, c_vp, c_vp]      # ctx, lut, x, x_stride, x_offset, dirs, n, y_est, stream
    L.amx_prep_predicted_device.argtypes = [c_vp, c_vp, c_vp, c_vp, C.c_int64, C.c_int64, c_vp, c_vp, c_vp, c_vp]   # ctx, plan, lut, x, x_stride, x_offset, dirs, mean_b0, volume, stream
    for f_ in (L.amx_bootstrap_resample_device, L.amx_bootstrap_resample_device_f32):
        f_.argtypes = [c_vp, c_vp, c_vp, C.c_int64, C.c_int, C.c_int64, C.c_uint64, C.c_int64, c_vp, c_vp]   # ctx, y, y_est, n, nS, first_voxel, seed, replicate, y_b, stream
    L.amx_bootstrap_accumulate_device.argtypes = [c_vp, c_vp, C.c_int64, C.c_int64, c_vp, c_vp, c_vp]              # ctx, maps, n_elems, t, mean, m2, stream
    L.amx_bootstrap_std_device.argtypes = [c_vp, c_vp, C.c_int64, C.c_int64, c_vp, c_vp]                           # ctx, m2, n_elems, B, std, stream
    L.amx_debug_fetch.argtypes = [c_vp, c_vp, C.c_int, c_vp, C.c_size_t]
    L.amx_set_progress.argtypes = [c_vp, PROGRESS_CB, c_vp]
    L.amx_lut_upload_czb.argtypes = [c_vp, c_fp, c_fp, c_fp, c_dp, c_i16p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(c_vp)]
    L.amx_set_profiling.argtypes = [c_vp, C.c_int]
    L.amx_last_kernel_ms.argtypes = [c_vp, C.c_int, C.POINTER(C.c_float)]
    L.amx_last_stats.argtypes = [c_vp, c_i64p]
    L.amx_last_seed_stats.argtypes = [c_vp, c_i64p]
    L.amx_last_host_narrowed.argtypes = [c_vp]
    L.amx_last_path.argtypes = [c_vp, C.c_char_p, C.c_int]
    L.amx_prep_route.argtypes = [C.c_int] * 7 + [c_i64p]
    L.amx_noddi_route.argtypes = [C.c_int] * 5 + [C.c_int64] * 2 + [C.c_double] * 2 + [C.c_char_p, C.c_int, c_i64p]
    L.amx_small_route.argtypes = [C.c_int] * 4 + [C.c_int64] + [C.c_double] * 2 + [C.c_uint, C.c_int, C.c_uint, C.c_char_p, C.c_int, c_i64p]
    L.amx_prep_last_launch.argtypes = [c_vp, C.c_char_p, C.c_int, c_i64p]
    L.amx_host_pool_info.argtypes = [c_vp, C.POINTER(C.c_int)]
    L.amx_set_call_voxels.argtypes = [c_vp, C.c_int64]
    L.amx_dict_upload.argtypes = [c_vp, c_dp, C.c_int, C.c_int, C.c_int, C.POINTER(c_vp)]
    L.amx_dict_destroy.argtypes = [c_vp]
    L.amx_dict_destroy.restype = None
    L.amx_dict_set_dense.argtypes = [c_vp, c_vp, C.c_int]
    L.amx_batched_last_dense.argtypes = [c_vp, c_i64p]
    L.amx_nnls_batched.argtypes = [c_vp, c_vp, c_i32p, c_dp, C.c_int64, c_dp, c_dp]
    L.amx_lasso_batched.argtypes = [c_vp, c_vp, c_i32p, c_dp, C.c_int64, C.c_double, C.c_double, c_dp]
    L.amx_nnls_batched_device.argtypes = [c_vp, c_vp, c_vp, c_vp, C.c_int64, c_vp, c_vp, c_vp]
    L.amx_lasso_batched_device.argtypes = [c_vp, c_vp, c_vp, c_vp, C.c_int64, C.c_double, C.c_double, c_vp, c_vp]
    L.amx_selftest.argtypes = [c_vp, c_dp]
    L.amx_dti_create.argtypes = [c_vp, c_dp, C.c_int, C.c_double, C.POINTER(c_vp)]
    L.amx_dti_create_method.argtypes = [c_vp, c_dp, c_dp, C.c_int, C.c_double, C.c_int, C.POINTER(c_vp)]
    L.amx_dti_create_robust.argtypes = [c_vp, c_dp, c_dp, C.c_int, C.c_double, C.c_double, C.POINTER(c_vp)]
    L.amx_dti_last_unconverged.argtypes = [c_vp, c_vp, C.POINTER(C.c_int64)]
    L.amx_dti_last_robust.argtypes = [c_vp, c_vp, C.POINTER(C.c_int64)]
    L.amx_dti_last_trips.argtypes = [c_vp, c_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.amx_dti_destroy.argtypes = [c_vp]
    L.amx_dti_destroy.restype = None
    L.amx_dti_directions.argtypes = [c_vp, c_vp, c_dp, C.c_int64, c_dp]
    L.amx_dti_directions_device.argtypes = [c_vp, c_vp, c_vp, C.c_int64, c_vp, c_vp]
    L.amx_dti_directions_device_f32.argtypes = [c_vp, c_vp, c_vp, C.c_int64, c_vp, c_vp]
    n_out = len(Dti.OUTPUTS)        # ctx, dti, y, n, min_diffusivity, one pointer per row of Dti.OUTPUTS (, stream)
    L.amx_dti_fit.argtypes = [c_vp, c_vp, c_dp, C.c_int64, C.c_double] + [c_dp] * n_out
    L.amx_dti_fit_device.argtypes = [c_vp, c_vp, c_vp, C.c_int64, C.c_double] + [c_vp] * (n_out + 1)
    L.amx_dti_fit_device_f32.argtypes = [c_vp, c_vp, c_vp, C.c_int64, C.c_double] + [c_vp] * (n_out + 1)
    # (the robust calls: the outlier counts int32 [n] behind the other outputs)
    L.amx_dti_fit_robust.argtypes = [c_vp, c_vp, c_dp, C.c_int64, C.c_double] + [c_dp] * n_out + [c_i32p]
    L.amx_dti_fit_robust_device.argtypes = [c_vp, c_vp, c_vp, C.c_int64, C.c_double] + [c_vp] * (n_out + 2)
    L.amx_dti_fit_robust_device_f32.argtypes = [c_vp, c_vp, c_vp, C.c_int64, C.c_double] + [c_vp] * (n_out + 2)
    L.amx_prep_create.argtypes = [c_vp, c_i64p, c_i64p, C.c_int, c_i32p, C.c_int64, c_i32p, c_i32p, C.c_int,
                                  c_i32p, C.c_int, C.c_int, C.POINTER(c_vp)]
    L.amx_prep_destroy.argtypes = [c_vp]
    L.amx_prep_destroy.restype = None
    L.amx_prep_gather.argtypes = [c_vp, c_vp, c_fp, C.c_int, C.c_float, c_dp, c_fp]
    L.amx_prep_gather_device.argtypes = [c_vp, c_vp, c_vp, C.c_int, C.c_float, c_vp, c_vp, c_vp]
    L.amx_prep_gather_device_f32.argtypes = [c_vp, c_vp, c_vp, C.c_int, C.c_float, c_vp, c_vp, c_vp]
    for f_ in (L.amx_prep_gather_directions_device, L.amx_prep_gather_directions_device_f32):
        f_.argtypes = [c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_float, c_vp, c_vp, c_vp, c_vp]      # ctx, plan, tensor helper, img, normalize, thr, y, mean_b0, dirs, stream
    L.amx_prep_mean_b0.argtypes = [c_vp, c_vp, c_fp, c_fp]
    L.amx_prep_mean_b0_device.argtypes = [c_vp, c_vp, c_vp, c_vp, c_vp]
    L.amx_prep_scatter.argtypes = [c_vp, c_vp, c_dp, C.c_int, c_fp]
    L.amx_prep_scatter_device.argtypes = [c_vp, c_vp, c_vp, C.c_int, c_vp, c_vp]
    L.amx_debias_rows.argtypes = [c_vp, c_dp, C.c_int64, C.c_int, c_i32p, C.c_int, C.c_double, c_dp]
    L.amx_debias_rows_f32.argtypes = [c_vp, c_fp, C.c_int64, C.c_int, c_i32p, C.c_int, C.c_double, c_dp]
    for f_ in (L.amx_debias_rows_device, L.amx_debias_rows_device_f32):
        f_.argtypes = [c_vp, c_vp, C.c_int64, C.c_int, c_i32p, C.c_int, C.c_double, c_vp, c_vp]      # ctx, S, n, nS, b0_idx (host), n_b0, snr, E, stream
    L.amx_prep_set_debias_mask.argtypes = [c_vp, c_vp, C.POINTER(C.c_uint8)]
    L.amx_prep_debias.argtypes = [c_vp, c_vp, c_fp, C.c_double]
    L.amx_prep_debias_device.argtypes = [c_vp, c_vp, c_vp, C.c_double, c_vp]
    L.amx_debias_last_unconverged.argtypes = [c_vp, C.POINTER(C.c_int64)]
    for f_ in (L.amx_noise_b0_rows_device, L.amx_noise_b0_rows_device_f32):
        f_.argtypes = [c_vp, c_vp, C.c_int64, C.c_int, c_i32p, C.c_int, c_vp, c_vp, c_vp, c_vp]      # ctx, S, n, nS, b0_idx (host), n_b0, mean, sd, ratio, stream
    L.amx_prep_noise_b0_device.argtypes = [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]                 # ctx, plan, img, mean, sd, ratio, stream
    L.amx_nanmedian_device.argtypes = [c_vp, c_vp, C.c_int64, c_vp, c_vp, c_vp]                      # ctx, v, n, out[2], count, stream
    L.amx_prep_noise_mppca_device.argtypes = [c_vp, c_vp, c_vp, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]   # ctx, plan, img, patch, sigma, n_signal, mean, ratio, eig, stream
    L.amx_mppca_route.argtypes = [C.c_int, C.c_int, C.c_int, c_i64p, c_i64p]                         # nS, patch, n_cols, dims[3], out[10]
    L.amx_prep_noise_mppca_denoise_device.argtypes = [c_vp, c_vp, c_vp, C.c_int] + [c_vp] * 8      # ctx, plan, img, patch, out, sigma, n_signal, mean, ratio, status, rows64, stream
    L.amx_mppca_denoise_route.argtypes = [C.c_int, C.c_int, C.c_int, c_i64p, c_i64p]                 # nS, patch, n_cols, dims[3], out[11]
    L.amx_prep_unring_device.argtypes = [c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, c_i64p, c_i64p, c_vp]   # ctx, plan, img, out, axis_a, axis_b, slices, passed_through, stream
    L.amx_unring_route.argtypes = [C.c_int, C.c_int, c_i64p]                                         # n_a, n_b, out[14]
    L.amx_prep_sanitize.argtypes = [c_vp, c_vp, c_fp, C.c_int, C.c_float, C.POINTER(C.c_int64)]
    L.amx_prep_sanitize_device.argtypes = [c_vp, c_vp, c_vp, C.c_int, C.c_float, c_vp]
    L.amx_sanitize_device_f32.argtypes = [c_vp, c_vp, C.c_int64, C.c_int, C.c_float, c_vp]
    L.amx_sanitize_device.argtypes = [c_vp, c_vp, C.c_int64, C.c_int, C.c_double, c_vp]
    L.amx_sanitize.argtypes = [c_vp, c_dp, C.c_int64, C.c_int, C.c_double, C.POINTER(C.c_int64)]
    L.amx_sanitize_last.argtypes = [c_vp, C.POINTER(C.c_int64)]
    L.amx_sanitize_previous.argtypes = [c_vp, C.POINTER(C.c_int64)]
    L.amx_prep_ingest_device.argtypes = [c_vp, c_vp, c_vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_float, c_vp, c_vp]   # ctx, plan, raw, dtype, slope, inter, replace, value, img, stream
    L.amx_prep_ingest.argtypes = [c_vp, c_vp, c_vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_float, c_fp, C.POINTER(C.c_int64)]
    L.amx_lut_resample.argtypes = [c_vp, c_fp, C.c_int64, C.c_int, c_fp, c_i32p, C.c_int, C.c_int, c_fp]
    L.amx_lut_rotate_resample.argtypes = [c_vp, c_fp, C.c_int, c_fp, C.c_int, C.c_int, C.c_int, c_fp, c_i32p, C.c_int, C.c_int, c_fp]
    L.amx_lut_route.argtypes = [C.c_int] * 3 + [c_i64p]
    _lib = L
    return L


def _p(a, ct):
    return a.ctypes.data_as(ct) if a is not None else None


def device_count():
    """gfx950 devices this process can see (amx_device_count; 0 without a usable GPU)"""
    return max(0, int(lib().amx_device_count()))


class Context:
    """amx_ctx: one per process and GPU."""

    def __init__(self, device=-1):
        self._h = c_vp()
        rc = lib().amx_ctx_create(int(device), C.byref(self._h))
        if rc != AMX_OK:
            self._h = None
            raise AmxError(rc, 'amico_amd: no usable MI355X (gfx950) device -- the fit path has no CPU fallback'
                           if rc == AMX_E_NODEVICE else f'amx_ctx_create failed ({rc})')

    def close(self):
        if getattr(self, '_h', None):
            lib().amx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc == AMX_OK:
            return
        msg = lib().amx_last_error(self._h).decode('utf-8', 'replace')
        if rc == AMX_E_BADARG:
            raise ValueError(msg or 'bad argument')
        raise AmxError(rc, msg or f'amico_amd error {rc}')       # RuntimeError, like lut.pyx:352-354

    def set_call_voxels(self, total):
        """the host-buffer fits that follow are shards of a call of `total` voxels (amx_set_call_voxels; 0 = off)"""
        self.check(lib().amx_set_call_voxels(self._h, int(total)))

    def sync(self, stream=None):
        self.check(lib().amx_sync_status(self._h, c_vp(stream or 0)))

    def set_progress(self, fn=None):
        """fn(done, total) is called while a host-buffer fit runs (batches of voxels complete); None unregisters"""
        self._progress_cb = PROGRESS_CB(lambda done, total, _u: fn(int(done), int(total))) if fn else PROGRESS_CB()
        self.check(lib().amx_set_progress(self._h, self._progress_cb, None))

    def set_profiling(self, on=True, only=None):
        """HIP events around the kernel groups of every fit (amx_last_kernel_ms); only=w: the pair of group w alone (each event is a packet
        of the stream: the full set costs a NODDI fit ~70 us)"""
        self.check(lib().amx_set_profiling(self._h, (2 + int(only)) if (on and only is not None) else int(bool(on))))

    def last_kernel_ms(self, which=0):
        ms = C.c_float()
        self.check(lib().amx_last_kernel_ms(self._h, int(which), C.byref(ms)))
        return ms.value

    def last_stats(self):
        out = (C.c_int64 * 4)()
        self.check(lib().amx_last_stats(self._h, out))
        return {'rerun_voxels': out[0], 'itercap_voxels': out[1], 'overflow_voxels': out[2],
                'guard_trips': out[3] >> 32, 'guard_last': out[3] & 0xffffffff}

    def debias_last_unconverged(self):
        """samples of the last debias call that reached the trip cap (amx_debias_last_unconverged; waits for that call)"""
        out = C.c_int64()
        self.check(lib().amx_debias_last_unconverged(self._h, C.byref(out)))
        return int(out.value)

    def sanitize_last(self):
        """NaN / Inf elements the last sanitize call on this context found (amx_sanitize_last; waits for that call)"""
        out = C.c_int64()
        self.check(lib().amx_sanitize_last(self._h, C.byref(out)))
        return int(out.value)

    def sanitize_previous(self):
        """... and the call before the last one (amx_sanitize_previous): a chain scans the image, then y, and reads both at its end"""
        out = C.c_int64()
        self.check(lib().amx_sanitize_previous(self._h, C.byref(out)))
        return int(out.value)

    def last_host_narrowed(self):
        """batches of the last host-buffer call whose float64 signals crossed PCIe as float32, losslessly (amx_last_host_narrowed)"""
        return int(lib().amx_last_host_narrowed(self._h))

    def host_pool_info(self):
        """host threads of the float32 transport of this context (amx_host_pool_info)"""
        out = (C.c_int * 4)()
        self.check(lib().amx_host_pool_info(self._h, out))
        return {'threads': out[0], 'first_cpu': out[1], 'physical_cores': out[2], 'device': out[3]}

    def last_path(self):
        """the kernels the last fit on this context enqueued, in launch order (amx_last_path)"""
        buf = C.create_string_buffer(2048)
        self.check(lib().amx_last_path(self._h, buf, 2048))
        return buf.value.decode()

    def last_dense(self):
        """what k_batched_big did in the last synchronised batched call (amx_batched_last_dense): the voxels of a dense dictionary whose
        support outgrew the 48-atom pass, and the pivoting steps they took together"""
        out = (C.c_int64 * 2)()
        self.check(lib().amx_batched_last_dense(self._h, out))
        return {'voxels': int(out[0]), 'steps': int(out[1])}

    def last_seed_stats(self):
        """how the NODDI voxels since the previous sync were settled (amx_last_seed_stats): certification rates of the three stages"""
        out = (C.c_int64 * 8)()
        self.check(lib().amx_last_seed_stats(self._h, out))
        n = int(out[0])
        d = {'seeded_voxels': n, 'leftover_stage1': int(out[1]), 'leftover_lasso': int(out[2]), 'leftover_stage3': int(out[3]),
             'clipped_stage2': int(out[4])}
        if n > 0:
            d['certified'] = [1.0 - out[k] / n for k in (1, 2, 3)]
        return d

    def selftest(self):
        out = np.zeros((12, 64))
        self.check(lib().amx_selftest(self._h, _p(out, c_dp)))
        return out


class Lut:
    """amx_lut: device-resident dictionary."""

    def __init__(self, ctx, handle, model, nS, n_atoms, n_maps=None, n_iso=None):
        self.ctx, self._h, self.model, self.nS, self.n_atoms, self.n_maps, self.n_iso = ctx, handle, model, nS, n_atoms, n_maps, n_iso

    def close(self):
        if getattr(self, '_h', None) and getattr(self.ctx, '_h', None):
            lib().amx_lut_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upload_noddi(ctx, kernels, htable, dwi_idx, is_exvivo=False):
    wm = np.ascontiguousarray(kernels['wm'], dtype=np.float32)
    if wm.ndim != 3:
        raise ValueError("KERNELS['wm'] must be [n_wm, ndirs, nS]")
    n_wm, ndirs, nS = wm.shape
    iso = np.ascontiguousarray(kernels['iso'], dtype=np.float32)
    norms = np.ascontiguousarray(kernels['norms'], dtype=np.float64)
    icvf = np.ascontiguousarray(kernels['icvf'], dtype=np.float32)
    kappa = np.ascontiguousarray(kernels['kappa'], dtype=np.float32)
    ht = np.ascontiguousarray(htable, dtype=np.int16)
    dwi = np.ascontiguousarray(dwi_idx, dtype=np.int64)
    if iso.shape != (nS,) or icvf.shape != (n_wm,) or kappa.shape != (n_wm,) or ht.size != 181 * 181 \
            or norms.shape != (len(dwi), n_wm):
        raise ValueError('NODDI KERNELS / htable have inconsistent shapes')
    h = c_vp()
    ctx.check(lib().amx_lut_upload_noddi(ctx._h, _p(wm, c_fp), _p(iso, c_fp), _p(norms, c_dp), _p(icvf, c_fp),
                                         _p(kappa, c_fp), _p(ht, c_i16p), _p(dwi, c_i64p), n_wm, ndirs, nS,
                                         len(dwi), int(bool(is_exvivo)), C.byref(h)))
    return Lut(ctx, h, 'NODDI', nS, n_wm + 1 + (1 if is_exvivo else 0), 3 + (1 if is_exvivo else 0))


def upload_freewater(ctx, kernels, htable):
    D = np.ascontiguousarray(kernels['D'], dtype=np.float32)
    CSF = np.ascontiguousarray(kernels['CSF'], dtype=np.float32)
    if D.ndim != 3 or CSF.ndim != 2 or CSF.shape[1] != D.shape[2]:
        raise ValueError('FreeWater KERNELS have inconsistent shapes')
    ht = np.ascontiguousarray(htable, dtype=np.int16)
    if ht.size != 181 * 181:
        raise ValueError('htable must have 181*181 entries')
    h = c_vp()
    ctx.check(lib().amx_lut_upload_freewater(ctx._h, _p(D, c_fp), _p(CSF, c_fp), _p(ht, c_i16p), D.shape[0],
                                             CSF.shape[0], D.shape[1], D.shape[2], C.byref(h)))
    return Lut(ctx, h, 'FreeWater', D.shape[2], D.shape[0] + CSF.shape[0], n_iso=CSF.shape[0])


def upload_sandi(ctx, kernels, Rs, d_in, d_isos):
    sig = np.asfortranarray(kernels['signal'], dtype=np.float64)
    norms = np.ascontiguousarray(kernels['norms'], dtype=np.float64)
    Rs = np.ascontiguousarray(Rs, dtype=np.float64)
    d_in = np.ascontiguousarray(d_in, dtype=np.float64)
    d_isos = np.ascontiguousarray(d_isos, dtype=np.float64)
    nS, n_atoms = sig.shape
    if n_atoms != len(Rs) + len(d_in) + len(d_isos) or norms.shape != (n_atoms,):
        raise ValueError('SANDI KERNELS have inconsistent shapes')
    h = c_vp()
    ctx.check(lib().amx_lut_upload_sandi(ctx._h, _p(sig, c_dp), _p(norms, c_dp), _p(Rs, c_dp), _p(d_in, c_dp),
                                         _p(d_isos, c_dp), nS, len(Rs), len(d_in), len(d_isos), C.byref(h)))
    return Lut(ctx, h, 'SANDI', nS, n_atoms, 6)


def upload_czb(ctx, kernels, Rs, htable):
    wmr = np.ascontiguousarray(kernels['wmr'], dtype=np.float32)
    wmh = np.ascontiguousarray(kernels['wmh'], dtype=np.float32)
    iso = np.ascontiguousarray(kernels['iso'], dtype=np.float32)
    Rs = np.ascontiguousarray(Rs, dtype=np.float64)
    if wmr.ndim != 3 or wmh.ndim != 3 or iso.ndim != 2 or wmh.shape[1:] != wmr.shape[1:] or iso.shape[1] != wmr.shape[2] \
            or Rs.shape != (wmr.shape[0],):
        raise ValueError('CylinderZeppelinBall KERNELS / Rs have inconsistent shapes')
    ht = np.ascontiguousarray(htable, dtype=np.int16)
    if ht.size != 181 * 181:
        raise ValueError('htable must have 181*181 entries')
    h = c_vp()
    ctx.check(lib().amx_lut_upload_czb(ctx._h, _p(wmr, c_fp), _p(wmh, c_fp), _p(iso, c_fp), _p(Rs, c_dp), _p(ht, c_i16p),
                                       wmr.shape[0], wmh.shape[0], iso.shape[0], wmr.shape[1], wmr.shape[2], C.byref(h)))
    return Lut(ctx, h, 'CylinderZeppelinBall', wmr.shape[2], wmr.shape[0] + wmh.shape[0] + iso.shape[0], 3)


def _check_y(y, nS):
    """float32 signals stay float32 (amx_*_fit_f32: the image dtype of the reference, half the PCIe bytes, same results);
    anything else is passed as float64 like evaluation.y"""
    y = np.ascontiguousarray(y, dtype=np.float32 if getattr(y, 'dtype', None) == np.float32 else np.float64)
    if y.ndim != 2 or y.shape[1] != nS:
        raise ValueError(f'y must be [n_vox, {nS}] float64 (or float32)')
    return y


def _check_dirs(dirs, n):
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)      # a copy is never modified (lut.pyx:335-338 quirk)
    if dirs.shape != (n, 3):
        raise ValueError('DIRs must be [n_vox, 3]')
    return dirs


def _outs(out, n, specs):
    """result arrays of a host fit: fresh zeros, or the caller's (`out`: a tuple like the fit's return value -- C-contiguous float64
    arrays of the right shape, e.g. row slices of the arrays a multi-device fit hands to its shards; None where a result is off)"""
    res = []
    for k, (shape, on) in enumerate(specs):
        if not on:
            res.append(None)
            continue
        a = None if out is None else out[k]
        if a is None:
            a = np.zeros((n,) + shape, dtype=np.float64, order='C')
        elif a.dtype != np.float64 or a.shape != (n,) + shape or not a.flags['C_CONTIGUOUS'] or not a.flags['WRITEABLE']:
            raise ValueError('out[%d] must be a writable C-contiguous float64 array of shape %s' % (k, ((n,) + shape,)))
        res.append(a)
    return res


def _switches(row, want):
    """(flags, [output k is on]) of a call"""
    flags, on = 0, []
    for o in row.outputs:
        on.append(o.key is None or bool(want.get(o.key)))
        if on[-1]:
            flags |= o.flag
    return flags, on


def _fit_host(row, ctx, lut, y, dirs, lambda1, lambda2, extras, want, out):
    """the host-buffer fit of `row`: extras as the row describes them, want: wrapper keyword -> bool, out: see _outs"""
    y = _check_y(y, lut.nS)
    n = y.shape[0]
    if row.dirs:
        dirs = _check_dirs(dirs, n)
    if row.check is not None:
        row.check(lut, extras)
    flags, on = _switches(row, want)
    res = _outs(out, n, [(o.shape(lut, extras), k) for o, k in zip(row.outputs, on)])
    f32 = y.dtype == np.float32
    fn = getattr(lib(), 'amx_%s_fit%s' % (row.stem, '_f32' if f32 else ''))
    args = [ctx._h, lut._h, _p(y, c_fp if f32 else c_dp)] + ([_p(dirs, c_dp)] if row.dirs else [])
    args += (n, float(lambda1), float(lambda2)) + tuple(extras[:len(row.extras)]) + (flags,)
    ctx.check(fn(*args, *[_p(a, c_dp) for a in res]))
    return tuple(res)


def noddi_fit(ctx, lut, y, dirs, lambda1, lambda2, n_maps, rmse=False, nrmse=False, mod=False, out=None):
    return _fit_host(FIT['noddi'], ctx, lut, y, dirs, lambda1, lambda2, (n_maps,), dict(rmse=rmse, nrmse=nrmse, mod=mod), out)


def freewater_fit(ctx, lut, y, dirs, lambda1, lambda2, is_mouse, rmse=False, nrmse=False, corrected=False, out=None):
    return _fit_host(FIT['freewater'], ctx, lut, y, dirs, lambda1, lambda2, (int(bool(is_mouse)),),
                     dict(rmse=rmse, nrmse=nrmse, corrected=corrected), out)


def sandi_fit(ctx, lut, y, lambda1, lambda2, rmse=False, nrmse=False, out=None):
    return _fit_host(FIT['sandi'], ctx, lut, y, None, lambda1, lambda2, (), dict(rmse=rmse, nrmse=nrmse), out)


def czb_fit(ctx, lut, y, dirs, lambda1, lambda2, rmse=False, nrmse=False, out=None):
    return _fit_host(FIT['czb'], ctx, lut, y, dirs, lambda1, lambda2, (), dict(rmse=rmse, nrmse=nrmse), out)


# ---- the same four fits on DEVICE-resident inputs (torch tensors used as plain device buffers); outputs are torch
#      tensors on the same device, enqueued on `stream`; the caller synchronises with ctx.sync(stream)
# `which` of amx_debug_fetch (include/amico_amd.h holds each table's layout and shape)
DEBUG_WHICH = dict(
    perm=0, ytil=1, seeds=2, ytil2=3, seeds2=4, cgemm=5, schunks=6, misc=7,                      # workspace of the last fit (lut = None)
    basis_U=10, basis_S=11, basis2_U=12, basis2_S=13, tiles=14, gram=15, gram_dwi=16,            # made at the upload
    screen_S=17, screen2_S=18, screen_kappa=19, screen_kappa0=20, screen2_kappa=21, screen2_kappa0=22,
    u2iso=23, rowdwi=24, colscale=25, s2_derive=26,
    fw_prep=30, czb_prep=31, sandi_prep=32, sandi_long_prep=33,                                  # made by the first fit at a lambda2
    dict_gram=40)                                                                                # `lut` is a Dict


def debug_fetch(ctx, lut, which, shape, dtype):
    """workspace / dictionary tables (include/amico_amd.h: amx_debug_fetch; which: a code or a name of DEBUG_WHICH) as a numpy array"""
    which = DEBUG_WHICH.get(which, which)
    out = np.empty(shape, dtype=dtype)
    ctx.check(lib().amx_debug_fetch(ctx._h, lut._h if lut is not None else None, int(which), out.ctypes.data_as(c_vp), out.nbytes))
    return out


def _dptr(t):
    return c_vp(t.data_ptr()) if t is not None else None


def _check_dev(lut, y_t, dirs_t=None):
    """the kernels index `y` with the dictionary's nS as the row stride and `DIRs` with stride 3: anything else
    would read foreign memory and return garbage maps without an error"""
    import torch
    if y_t.dtype not in (torch.float64, torch.float32) or y_t.dim() != 2 or y_t.shape[1] != lut.nS or not y_t.is_contiguous():
        raise ValueError(f'y must be a contiguous float64 (or float32) device tensor [n_vox, {lut.nS}] (the dictionary was built for '
                         f'{lut.nS} volumes per voxel)')
    if dirs_t is not None and (dirs_t.dtype != torch.float64 or tuple(dirs_t.shape) != (y_t.shape[0], 3)
                               or not dirs_t.is_contiguous() or dirs_t.device != y_t.device):
        raise ValueError('DIRs must be a contiguous float64 device tensor [n_vox, 3] on the device of y')


def _own_tensor(name, t, shape, like):
    """a result tensor the caller hands in: checked as strictly as _outs checks host arrays"""
    import torch
    if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != like.device:
        raise ValueError('%s must be a contiguous float64 device tensor of shape %s on the device of y' % (name, (shape,)))
    return t


_NOTHING = contextlib.nullcontext()


@contextlib.contextmanager
def _fw_iso(ctx, xi):
    """the buffer AMX_F_FW_ISO writes to is registered for the length of the fit call"""
    ctx.check(lib().amx_set_fw_iso(ctx._h, _dptr(xi)))
    try:
        yield
    finally:
        lib().amx_set_fw_iso(ctx._h, None)       # (the kernels enqueued meanwhile carry the pointer; the tensor is the caller's from here)


def _fit_device(row, ctx, lut, y_t, dirs_t, lambda1, lambda2, extras, want, stream, return_x, iso, into=None):
    """the device-resident fit of `row` (extras, want: as for _fit_host).  return_x: the zeroed AMX_F_DEBUG_X coefficients come back behind
    the outputs; iso (Free-Water): True, or the tensor to write them into -- the isotropic coefficients f64 [n_vox, n_iso] come back
    last; into: the `estimates` tensor, when the caller owns one already"""
    import torch
    _check_dev(lut, y_t, dirs_t if row.dirs else None)
    if row.check is not None:
        row.check(lut, extras)
    n, f64 = y_t.shape[0], dict(dtype=torch.float64, device=y_t.device)
    (flags, on), xd, xi = _switches(row, want), None, None
    if return_x:
        xd = torch.zeros((n,) + row.x_shape(lut), **f64)
        ctx.check(lib().amx_set_debug_x(ctx._h, _dptr(xd)))
        flags |= F_DEBUG_X
    if iso is not False:
        xi = torch.empty((n, lut.n_iso), **f64) if iso is True else _own_tensor('iso', iso, (n, lut.n_iso), y_t)
        flags |= F_FW_ISO
    res = [torch.empty((n,) + o.shape(lut, extras), **f64) if k and not (o.key is None and into is not None) else None
           for o, k in zip(row.outputs, on)]
    if into is not None:
        res[0] = _own_tensor('into', into, (n,) + row.outputs[0].shape(lut, extras), y_t)
    fn = getattr(lib(), 'amx_%s_fit_device%s' % (row.stem, '_f32' if y_t.dtype == torch.float32 else ''))
    args = [ctx._h, lut._h, _dptr(y_t)] + ([_dptr(dirs_t)] if row.dirs else [])
    args += (n, float(lambda1), float(lambda2)) + tuple(extras[:len(row.extras)]) + (flags,)
    with _fw_iso(ctx, xi) if xi is not None else _NOTHING:
        ctx.check(fn(*args, *[_dptr(t) for t in res], c_vp(stream or 0)))
    return tuple(res) + ((xd,) if return_x else ()) + ((xi,) if xi is not None else ())


def noddi_fit_device(ctx, lut, y_t, dirs_t, lambda1, lambda2, n_maps, rmse=False, nrmse=False, mod=False, stream=None,
                     return_x=False):
    return _fit_device(FIT['noddi'], ctx, lut, y_t, dirs_t, lambda1, lambda2, (n_maps,), dict(rmse=rmse, nrmse=nrmse, mod=mod), stream,
                       return_x, False)


def freewater_fit_device(ctx, lut, y_t, dirs_t, lambda1, lambda2, is_mouse, rmse=False, nrmse=False, corrected=False,
                         stream=None, return_x=False, iso=False):
    """iso=True: the isotropic coefficients of every voxel, f64 [n_vox, n_iso], come back as one more element (AMX_F_FW_ISO: what
    freewater_corrected_device / Prep.corrected_device make the corrected DWI from; the flag changes no path, unlike corrected=True)"""
    return _fit_device(FIT['freewater'], ctx, lut, y_t, dirs_t, lambda1, lambda2, (int(bool(is_mouse)),),
                       dict(rmse=rmse, nrmse=nrmse, corrected=corrected), stream, return_x, bool(iso))


def czb_fit_device(ctx, lut, y_t, dirs_t, lambda1, lambda2, rmse=False, nrmse=False, stream=None, return_x=False):
    return _fit_device(FIT['czb'], ctx, lut, y_t, dirs_t, lambda1, lambda2, (), dict(rmse=rmse, nrmse=nrmse), stream, return_x, False)


def sandi_fit_device(ctx, lut, y_t, lambda1, lambda2, rmse=False, nrmse=False, stream=None, return_x=False):
    return _fit_device(FIT['sandi'], ctx, lut, y_t, None, lambda1, lambda2, (), dict(rmse=rmse, nrmse=nrmse), stream, return_x, False)


def freewater_corrected_device(ctx, lut, y_t, xiso_t, stream=None, into=None):
    """y f32 | f64 [n, nS] and x_iso f64 [n, n_iso] (device tensors) -> y_corrected f64 [n, nS] (models.pyx:1264-1274): the rows
    AMX_F_CORRECTED writes, from the coefficients a fit with iso=True left (amx_freewater_corrected_device); enqueued on `stream`.
    into: the float64 device tensor [n, nS] to write (default: a new one)"""
    import torch
    _check_dev(lut, y_t)
    n = y_t.shape[0]
    if xiso_t.dtype != torch.float64 or tuple(xiso_t.shape) != (n, lut.n_iso) or not xiso_t.is_contiguous() or xiso_t.device != y_t.device:
        raise ValueError(f'x_iso must be a contiguous float64 device tensor [n_vox, {lut.n_iso}] on the device of y')
    yc = into
    if yc is None:
        yc = torch.empty((n, lut.nS), dtype=torch.float64, device=y_t.device)
    elif yc.dtype != torch.float64 or tuple(yc.shape) != (n, lut.nS) or not yc.is_contiguous() or yc.device != y_t.device:
        raise ValueError(f'into must be a contiguous float64 device tensor [n_vox, {lut.nS}] on the device of y')
    f32 = y_t.dtype == torch.float32
    ctx.check(lib().amx_freewater_corrected_device(ctx._h, lut._h, _dptr(y_t) if f32 else None, None if f32 else _dptr(y_t), _dptr(xiso_t),
                                                   n, _dptr(yc), c_vp(stream or 0)))
    return yc


def _check_x(lut, x_t, dirs_t, n=None):
    """(x_stride, x_offset) of a coefficient tensor: f64 [n, n_atoms], or NODDI's AMX_F_DEBUG_X layout [n, 3, n_atoms] (row 2 is taken)"""
    import torch
    na = lut.n_atoms
    if x_t.dtype != torch.float64 or not x_t.is_contiguous() or tuple(x_t.shape[1:]) not in ((na,), (3, na)) or (n is not None and x_t.shape[0] != n):
        raise ValueError(f'x must be a contiguous float64 device tensor [n_vox, {na}] (or [n_vox, 3, {na}], the NODDI layout of return_x)')
    if dirs_t is not None and (dirs_t.dtype != torch.float64 or tuple(dirs_t.shape) != (x_t.shape[0], 3) or not dirs_t.is_contiguous()
                               or dirs_t.device != x_t.device):
        raise ValueError('DIRs must be a contiguous float64 device tensor [n_vox, 3] on the device of x')
    return (3 * na, 2 * na) if x_t.dim() == 3 else (na, 0)


def predict_device(ctx, lut, x_t, dirs_t=None, stream=None):
    """the signal the fitted model predicts, y_est = A x, f64 [n, nS] (amx_predict_device): x_t the coefficients a fit with return_x=True
    left -- f64 [n, n_atoms], or NODDI's [n, 3, n_atoms] whose debiased row is taken --, dirs_t the directions of that fit (None for
    SANDI); fp64, one rounding per product and sum, atoms ascending.  Device tensors, enqueued on `stream`"""
    import torch
    stride, offset = _check_x(lut, x_t, dirs_t)
    n = x_t.shape[0]
    ye = torch.empty((n, lut.nS), dtype=torch.float64, device=x_t.device)
    ctx.check(lib().amx_predict_device(ctx._h, lut._h, _dptr(x_t), stride, offset, _dptr(dirs_t), n, _dptr(ye), c_vp(stream or 0)))
    return ye


def _f64_like(name, t, like, shape=None):
    import torch
    if t.dtype != torch.float64 or not t.is_contiguous() or t.device != like.device or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError('%s must be a contiguous float64 device tensor%s on the device of the other arguments'
                         % (name, '' if shape is None else ' of shape %s' % (tuple(shape),)))
    return t


def bootstrap_resample_device(ctx, y_t, yest_t, seed, replicate, first_voxel=0, stream=None, into=None):
    """one wild-bootstrap replicate of the signals (amx_bootstrap_resample_device[_f32]): y_b = max(0, y_est + s (y - y_est)) with the
    Rademacher sign s of (seed, replicate, first_voxel + i, j, nS) -- include/amico_amd.h has the generator.  y_t f32 | f64 [n, nS],
    yest_t f64 [n, nS] (predict_device); the replicate has the dtype of y.  into: the tensor to write (it must not be y or y_est)"""
    import torch
    if y_t.dtype not in (torch.float64, torch.float32) or y_t.dim() != 2 or not y_t.is_contiguous():
        raise ValueError('y must be a contiguous float64 (or float32) device tensor [n_vox, nS]')
    _f64_like('y_est', yest_t, y_t, y_t.shape)
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError('seed must be an integer in 0 .. 2^64 - 1')
    yb = into
    if yb is None:
        yb = torch.empty_like(y_t)
    elif yb.dtype != y_t.dtype or yb.shape != y_t.shape or not yb.is_contiguous() or yb.device != y_t.device:
        raise ValueError('into must be a contiguous device tensor of the shape and dtype of y, on its device')
    fn = lib().amx_bootstrap_resample_device_f32 if y_t.dtype == torch.float32 else lib().amx_bootstrap_resample_device
    ctx.check(fn(ctx._h, _dptr(y_t), _dptr(yest_t), y_t.shape[0], y_t.shape[1], int(first_voxel), int(seed), int(replicate), _dptr(yb),
                 c_vp(stream or 0)))
    return yb


def bootstrap_accumulate_device(ctx, maps_t, t, mean_t, m2_t, stream=None):
    """Welford's step for the t-th replicate's maps (t from 1; amx_bootstrap_accumulate_device): mean_t / m2_t are updated in place"""
    _f64_like('mean', mean_t, maps_t, maps_t.shape)
    _f64_like('M2', m2_t, maps_t, maps_t.shape)
    _f64_like('maps', maps_t, mean_t)
    ctx.check(lib().amx_bootstrap_accumulate_device(ctx._h, _dptr(maps_t), maps_t.numel(), int(t), _dptr(mean_t), _dptr(m2_t),
                                                    c_vp(stream or 0)))


def bootstrap_std_device(ctx, m2_t, samples, stream=None, into=None):
    """std = sqrt(M2 / (samples - 1)) (amx_bootstrap_std_device); into: the tensor to write (default: a new one)"""
    import torch
    sd = torch.empty_like(m2_t) if into is None else _f64_like('into', into, m2_t, m2_t.shape)
    _f64_like('M2', m2_t, sd)
    ctx.check(lib().amx_bootstrap_std_device(ctx._h, _dptr(m2_t), m2_t.numel(), int(samples), _dptr(sd), c_vp(stream or 0)))
    return sd


class Dict:
    """amx_dict: the dictionaries of the batched solver entry points (cyspams.interfaces.nnls / lasso, models.pyx:18, batched).
    A: [n_dicts, m, n] (or [m, n]) in numpy's own layout -- the column-major m x n slices the C ABI wants are made here.
    dense=True (or set_dense(True) later) also keeps the Gram matrices of the dictionaries in HBM (n^2 doubles each): on such a dictionary
    no voxel is refused for the size of its support (amx_dict_set_dense); the default refuses supports of more than 48 atoms."""

    def __init__(self, ctx, A, dense=False):
        A = np.asarray(A, dtype=np.float64)
        if A.ndim == 2:
            A = A[None]
        if A.ndim != 3:
            raise ValueError('dictionary must be [m, n] or [n_dicts, m, n]')
        self.ctx, (self.n_dicts, self.m, self.n) = ctx, A.shape
        cm = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))          # [n_dicts][n][m]: column-major m x n per dictionary
        h = c_vp()
        ctx.check(lib().amx_dict_upload(ctx._h, _p(cm, c_dp), self.m, self.n, self.n_dicts, C.byref(h)))
        self._h = h
        self.dense = False
        if dense:
            self.set_dense(True)

    def set_dense(self, on=True, ctx=None):
        """build (on) or free (off) the Gram tables; ctx: the context to call through (the dictionary's own)"""
        (ctx or self.ctx).check(lib().amx_dict_set_dense((ctx or self.ctx)._h, self._h, int(bool(on))))
        self.dense = bool(on)

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                lib().amx_dict_destroy(self._h)
                self._h = None
        except Exception:
            pass


def _batched_inputs(dic, y, idx):
    y = np.ascontiguousarray(np.atleast_2d(y), dtype=np.float64)
    if y.shape[1] != dic.m:
        raise ValueError(f'y has {y.shape[1]} samples, the dictionary {dic.m}')
    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.shape != (y.shape[0],):
            raise ValueError('dict_idx must have one entry per voxel')
    elif dic.n_dicts != 1:
        raise ValueError('dict_idx is required with more than one dictionary')
    return y, idx


def nnls_batched(ctx, dic, y, dict_idx=None, return_rnorm=False):
    """x_v = argmin_{x >= 0} ||A_d x - y_v||, d = dict_idx[v]: (X [n_vox, n], rnorm [n_vox]) -- models.pyx:911, 940"""
    y, idx = _batched_inputs(dic, y, dict_idx)
    x = np.zeros((y.shape[0], dic.n))
    rn = np.zeros(y.shape[0]) if return_rnorm else None
    ctx.check(lib().amx_nnls_batched(ctx._h, dic._h, _p(idx, c_i32p) if idx is not None else None, _p(y, c_dp), y.shape[0], _p(x, c_dp),
                                     _p(rn, c_dp) if rn is not None else None))
    return (x, rn) if return_rnorm else x


def lasso_batched(ctx, dic, y, lambda1, lambda2, dict_idx=None):
    """x_v = argmin_{x >= 0} 1/2 ||y_v - A_d x||^2 + lambda1 sum(x) + lambda2 / 2 ||x||^2 -- models.pyx:615, 926, 1238, 1569"""
    y, idx = _batched_inputs(dic, y, dict_idx)
    x = np.zeros((y.shape[0], dic.n))
    ctx.check(lib().amx_lasso_batched(ctx._h, dic._h, _p(idx, c_i32p) if idx is not None else None, _p(y, c_dp), y.shape[0],
                                      float(lambda1), float(lambda2), _p(x, c_dp)))
    return x


def dir_to_lut_idx(ctx, lut, dirs):
    dirs = np.ascontiguousarray(np.atleast_2d(dirs), dtype=np.float64)
    out = np.zeros(dirs.shape[0], dtype=np.int32)
    ctx.check(lib().amx_dir_to_lut_idx(ctx._h, lut._h, _p(dirs, c_dp), dirs.shape[0], _p(out, c_i32p)))
    return out


def check_sigma(sigma):
    """the noise level of the robust tensor fit: a finite number > 0 (ValueError otherwise), as a float"""
    try:
        ok = not isinstance(sigma, (bool, str, bytes)) and np.ndim(sigma) == 0 and np.isfinite(float(sigma)) and float(sigma) > 0.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('sigma (the noise level of the robust tensor fit) must be a finite number > 0, got %r' % (sigma,))
    return float(sigma)


class Dti:
    """amx_dti: principal-direction estimator of one acquisition scheme (include/amico_amd.h, row f1)."""

    METHODS = {'OLS': 0, 'WLS': 1, 'NLLS': 2, 'RESTORE': 3}        # AMX_DTI_* (include/amico_amd.h)
    # the outputs of amx_dti_fit* in ABI order: (name, values per voxel); all float64.  scalars = FA, MD, AD, RD
    OUTPUTS = (('directions', 3), ('evals', 3), ('scalars', 4))

    def __init__(self, ctx, inv_design, min_signal=1e-4, design=None, method='OLS', sigma=None):
        """sigma: the noise level of 'RESTORE', in the units of the signal (a finite number > 0); None for the other methods"""
        w = np.ascontiguousarray(inv_design, dtype=np.float64)
        if w.ndim != 2 or w.shape[0] != 7:
            raise ValueError('inv_design must be pinv(design matrix), shape [7, nS]')
        if method not in self.METHODS:
            raise ValueError("method must be one of 'OLS', 'WLS', 'NLLS', 'RESTORE'")
        if method == 'RESTORE':
            sigma = check_sigma(sigma)
        elif sigma is not None:
            raise ValueError('sigma belongs to the RESTORE method')
        if design is None:
            if method != 'OLS':
                raise ValueError('%s needs the design matrix, shape [nS, 7]' % method)
            x = None
        else:
            x = np.ascontiguousarray(design, dtype=np.float64)
            if x.shape != (w.shape[1], 7):
                raise ValueError('design must be the design matrix, shape [nS, 7] = [%d, 7]' % w.shape[1])
        self.ctx, self.nS, self.method = ctx, w.shape[1], method
        self.sigma = sigma
        self._h = c_vp()
        if method == 'RESTORE':
            ctx.check(lib().amx_dti_create_robust(ctx._h, _p(x, c_dp), _p(w, c_dp), self.nS, float(min_signal), sigma, C.byref(self._h)))
        else:
            ctx.check(lib().amx_dti_create_method(ctx._h, None if x is None else _p(x, c_dp), _p(w, c_dp), self.nS, float(min_signal),
                                                  self.METHODS[method], C.byref(self._h)))

    def last_unconverged(self):
        """voxels of the last NLLS call that kept their starting parameters (waits for the call)"""
        out = C.c_int64(0)
        self.ctx.check(lib().amx_dti_last_unconverged(self.ctx._h, self._h, C.byref(out)))
        return out.value

    def last_trips(self):
        """(Levenberg-Marquardt trips summed over the voxels, trips their wavefronts ran for them) of the last NLLS call"""
        a, b = C.c_int64(0), C.c_int64(0)
        self.ctx.check(lib().amx_dti_last_trips(self.ctx._h, self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_robust(self):
        """(voxels that entered the reweighted fit, voxels refitted without their outliers, voxels at the reweighted fit's trip cap or
        give-up, voxels left with fewer than 7 inliers) of the last RESTORE call; zeros for the other methods"""
        out = (C.c_int64 * 4)()
        self.ctx.check(lib().amx_dti_last_robust(self.ctx._h, self._h, out))
        return tuple(int(v) for v in out)

    def close(self):
        if getattr(self, '_h', None) and getattr(self.ctx, '_h', None):
            lib().amx_dti_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def directions(self, y):
        """y f64[n_vox, nS] (host) -> f64[n_vox, 3]."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim != 2 or y.shape[1] != self.nS:
            raise ValueError('y must be [n_vox, %d]' % self.nS)
        out = np.zeros((y.shape[0], 3))
        self.ctx.check(lib().amx_dti_directions(self.ctx._h, self._h, _p(y, c_dp), y.shape[0], _p(out, c_dp)))
        return out

    def directions_device(self, d_y, n_vox, d_dirs, stream=None, f32=False):
        """device pointers (ints), enqueued on `stream`; check with ctx.sync(stream).  f32: d_y holds float32 signals."""
        fn = lib().amx_dti_directions_device_f32 if f32 else lib().amx_dti_directions_device
        self.ctx.check(fn(self.ctx._h, self._h, c_vp(d_y), int(n_vox), c_vp(d_dirs), c_vp(stream or 0)))

    def fit(self, y, min_diffusivity, want=None):
        """y f64[n_vox, nS] (host) -> {name: f64[n_vox, k]} for the rows of OUTPUTS named in `want` (default: all) -- amx_dti_fit"""
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim != 2 or y.shape[1] != self.nS:
            raise ValueError('y must be [n_vox, %d]' % self.nS)
        want = [name for name, _ in self.OUTPUTS] if want is None else list(want)
        unknown = [w for w in want if w not in dict(self.OUTPUTS)]
        if unknown or not want:
            raise ValueError('want must name some of %s' % ', '.join(name for name, _ in self.OUTPUTS))
        out = {name: np.zeros((y.shape[0], k)) for name, k in self.OUTPUTS if name in want}
        ptrs = [_p(out[name], c_dp) if name in out else None for name, _ in self.OUTPUTS]
        if self.method == 'RESTORE':
            # (the robust estimator: also 'outliers' int32 [n_vox], the samples its verdict left out -- amx_dti_fit_robust)
            out['outliers'] = np.zeros(y.shape[0], dtype=np.int32)
            self.ctx.check(lib().amx_dti_fit_robust(self.ctx._h, self._h, _p(y, c_dp), y.shape[0], float(min_diffusivity), *ptrs,
                                                    _p(out['outliers'], c_i32p)))
        else:
            self.ctx.check(lib().amx_dti_fit(self.ctx._h, self._h, _p(y, c_dp), y.shape[0], float(min_diffusivity), *ptrs))
        return out

    def fit_device(self, d_y, n_vox, min_diffusivity, d_dirs=None, d_evals=None, d_scalars=None, stream=None, f32=False,
                   d_outliers=None):
        """directions_device with the eigenvalues f64 [n_vox, 3] and FA, MD, AD, RD f64 [n_vox, 4]; a pointer of None (or 0) leaves that
        output out, and with d_evals and d_scalars both None this is directions_device (amx_dti_fit_device[_f32]).  d_outliers
        int32 [n_vox]: a RESTORE estimator's outlier counts (amx_dti_fit_robust_device[_f32])"""
        if d_outliers and self.method != 'RESTORE':
            raise ValueError('d_outliers belongs to a RESTORE estimator')
        ptrs = [c_vp(p or 0) for p in (d_dirs, d_evals, d_scalars)]
        if d_outliers:
            fn = lib().amx_dti_fit_robust_device_f32 if f32 else lib().amx_dti_fit_robust_device
            ptrs.append(c_vp(d_outliers))
        else:
            fn = lib().amx_dti_fit_device_f32 if f32 else lib().amx_dti_fit_device
        self.ctx.check(fn(self.ctx._h, self._h, c_vp(d_y), int(n_vox), float(min_diffusivity), *ptrs, c_vp(stream or 0)))


class Prep:
    """amx_prep: signal-preparation / result-scatter plan of one image geometry + mask + volume grouping."""

    def __init__(self, ctx, shape, strides, rank, groups, b0_idx, overwrite_in_order=False):
        """shape (X, Y, Z, nS); strides = element strides of the float32 image; rank int32[X, Y, Z] (C order);
        groups = list of index lists (one per output volume)."""
        self.ctx = ctx
        self.shape = tuple(int(v) for v in shape)
        self.strides = tuple(int(v) for v in strides)
        dims = np.asarray(self.shape[:3], dtype=np.int64)
        st = np.asarray(self.strides, dtype=np.int64)
        rank = np.ascontiguousarray(rank, dtype=np.int32)
        if rank.shape != self.shape[:3]:
            raise ValueError('rank must have the spatial shape of the image')
        self.n_vox = int((rank >= 0).sum())
        gptr = np.zeros(len(groups) + 1, dtype=np.int32)
        gptr[1:] = np.cumsum([len(g) for g in groups])
        gidx = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.int32).ravel() for g in groups]), dtype=np.int32)
        b0 = np.ascontiguousarray(b0_idx, dtype=np.int32)
        self.n_out = len(groups)
        self.n_b0 = len(b0)
        self.extent =1 + sum((d - 1) * s for d, s in zip(self.shape, self.strides))
        self._h = c_vp()
        ctx.check(lib().amx_prep_create(ctx._h, _p(dims, c_i64p), _p(st, c_i64p), self.shape[3], _p(rank, c_i32p),
                                        self.n_vox, _p(gptr, c_i32p), _p(gidx, c_i32p), self.n_out,
                                        _p(b0, c_i32p) if len(b0) else None, len(b0), int(bool(overwrite_in_order)),
                                        C.byref(self._h)))

    def close(self):
        if getattr(self, '_h', None) and getattr(self.ctx, '_h', None):
            lib().amx_prep_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _img_buffer(self, img):
        """the float32 image as the flat element buffer the strides refer to (no copy for C / Fortran arrays)"""
        if img.dtype != np.float32 or img.shape != self.shape or \
                tuple(s // 4 for s in img.strides) != self.strides:
            raise ValueError('image does not match the plan (dtype float32, shape, strides)')
        flat = np.lib.stride_tricks.as_strided(img, shape=(self.extent,), strides=(4,))
        return flat

    def last_launch(self):
        """-> (kernel name, workgroups, threads per workgroup, LDS bytes) of the plan's last gather (amx_prep_last_launch)"""
        buf = C.create_string_buffer(128)
        out = np.zeros(3, dtype=np.int64)
        self.ctx.check(lib().amx_prep_last_launch(self._h, buf, 128, _p(out, c_i64p)))
        return (buf.value.decode(),) + tuple(int(v) for v in out)

    def gather(self, img, normalize=True, b0_threshold=0.0):
        buf = self._img_buffer(img)
        y = np.zeros((self.n_vox, self.n_out))
        mb0 = np.zeros(self.n_vox, dtype=np.float32)
        self.ctx.check(lib().amx_prep_gather(self.ctx._h, self._h, _p(buf, c_fp), int(bool(normalize)),
                                             float(b0_threshold), _p(y, c_dp), _p(mb0, c_fp)))
        return y, (mb0 if normalize else None)

    def mean_b0(self, img):
        buf = self._img_buffer(img)
        out = np.zeros(self.shape[:3], dtype=np.float32)
        self.ctx.check(lib().amx_prep_mean_b0(self.ctx._h, self._h, _p(buf, c_fp), _p(out, c_fp)))
        return out

    def set_debias_mask(self, mask):
        """mask [X, Y, Z] as given to load_data: the voxels debiasRician works on are those != 0 (preproc.py:29)"""
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != self.shape[:3]:
            raise ValueError('mask must have the spatial shape of the image')
        self.ctx.check(lib().amx_prep_set_debias_mask(self.ctx._h, self._h, _p(m, C.POINTER(C.c_uint8))))

    def debias(self, img, snr):
        """host image, IN PLACE: float32(E) where the mask is nonzero, 0 elsewhere (amx_prep_debias)"""
        buf = self._img_buffer(img)
        if not img.flags.writeable:
            raise ValueError('the image is debiased in place and must be writeable')
        self.ctx.check(lib().amx_prep_debias(self.ctx._h, self._h, _p(buf, c_fp), float(snr)))
        return img

    def gather_device(self, d_img, d_y, d_mean_b0, normalize, b0_threshold=0.0, stream=None):
        """device pointers (ints): image -> float32 rows y [n_vox, n_out] and mean_b0 [n_vox] (amx_prep_gather_device_f32); enqueued on `stream`"""
        self.ctx.check(lib().amx_prep_gather_device_f32(self.ctx._h, self._h, c_vp(d_img), int(bool(normalize)), float(b0_threshold),
                                                        c_vp(d_y), c_vp(d_mean_b0), c_vp(stream or 0)))

    def gather_directions_device(self, dti, d_img, d_y, d_mean_b0, d_dirs, normalize, b0_threshold=0.0, stream=None):
        """gather_device and the principal directions f64 [n_vox, 3] of `dti` (a Dti) in one pass over the image
        (amx_prep_gather_directions_device_f32)"""
        self.ctx.check(lib().amx_prep_gather_directions_device_f32(self.ctx._h, self._h, dti._h, c_vp(d_img), int(bool(normalize)),
                                                                   float(b0_threshold), c_vp(d_y), c_vp(d_mean_b0), c_vp(d_dirs), c_vp(stream or 0)))

    def scatter_device(self, d_values, k, d_volume, stream=None):
        """device pointers (ints): f64 [n_vox, k] -> float32 volume [X, Y, Z, k], zero outside the mask (amx_prep_scatter_device)"""
        self.ctx.check(lib().amx_prep_scatter_device(self.ctx._h, self._h, c_vp(d_values), int(k), c_vp(d_volume), c_vp(stream or 0)))

    def mean_b0_device(self, d_img, d_volume, stream=None):
        """device pointers (ints): the b0 mean of every voxel, float32 [X, Y, Z] (amx_prep_mean_b0_device)"""
        self.ctx.check(lib().amx_prep_mean_b0_device(self.ctx._h, self._h, c_vp(d_img), c_vp(d_volume), c_vp(stream or 0)))

    def debias_device(self, d_img, snr, stream=None):
        """device pointer (int) of the image's element buffer, in place, enqueued on `stream`"""
        self.ctx.check(lib().amx_prep_debias_device(self.ctx._h, self._h, c_vp(d_img), float(snr), c_vp(stream or 0)))

    def noise_b0_device(self, d_img, d_mean=None, d_sd=None, d_ratio=None, stream=None):
        """device pointers (ints): the image's element buffer -> mean, sample standard deviation (ddof = 1) and mean / sd of the b0
        repeats of the voxels with mask == 1, f64 [n_vox] each in the plan's masked order, NaN where a voxel is not eligible; any of the
        three may be None, not all (amx_prep_noise_b0_device); enqueued on `stream`"""
        self.ctx.check(lib().amx_prep_noise_b0_device(self.ctx._h, self._h, c_vp(d_img), c_vp(d_mean or 0), c_vp(d_sd or 0), c_vp(d_ratio or 0),
                                                      c_vp(stream or 0)))

    def noise_mppca_device(self, d_img, patch=5, d_sigma=None, d_nsignal=None, d_mean=None, d_ratio=None, d_eig=None, stream=None):
        """device pointers (ints): the image's element buffer -> per voxel of mask == 1 the Marchenko-Pastur noise level of its patch of
        edge `patch` (3 | 5), the number of signal components, the b0 mean and mean / sigma, f64 [n_vox] each in the plan's masked order, and
        the Gram matrix' eigenvalues f64 [n_vox, 125] (ascending, then NaN); NaN where a voxel is not eligible; any may be None, not all
        (amx_prep_noise_mppca_device); enqueued on `stream`"""
        self.ctx.check(lib().amx_prep_noise_mppca_device(self.ctx._h, self._h, c_vp(d_img), int(patch), c_vp(d_sigma or 0), c_vp(d_nsignal or 0),
                                                         c_vp(d_mean or 0), c_vp(d_ratio or 0), c_vp(d_eig or 0), c_vp(stream or 0)))

    def unring_device(self, d_img, d_out, axes=(0, 1), stream=None):
        """device pointers (ints): the image's element buffer -> d_out, float32 in the image's layout and extent (no part of d_img): every
        slice along `axes` (two different axes out of 0, 1, 2 of the plan's shape, each extent 8 .. 256) with its Gibbs ringing removed by
        local sub-voxel shifts; a slice with a NaN / Inf sample is copied through (amx_prep_unring_device).  Enqueued on `stream`; waits
        for the last chunk -> (slices, passed_through)"""
        out = np.zeros(2, dtype=np.int64)
        self.ctx.check(lib().amx_prep_unring_device(self.ctx._h, self._h, c_vp(d_img), c_vp(d_out), int(axes[0]), int(axes[1]),
                                                    _p(out[0:1], c_i64p), _p(out[1:2], c_i64p), c_vp(stream or 0)))
        return int(out[0]), int(out[1])

    def noise_mppca_denoise_device(self, d_img, patch, d_out, d_sigma=None, d_nsignal=None, d_mean=None, d_ratio=None, d_status=None,
                                   d_rows64=None, stream=None):
        """device pointers (ints): the image's element buffer -> d_out, float32 in the image's layout and extent (no part of d_img): per
        voxel of mask == 1 that is eligible the centre's column of its patch's best approximation of rank n_signal, every other sample
        the image's; sigma, n_signal, mean, ratio as `noise_mppca_device` writes them; d_status int32 [n_vox] (0 denoised, 1 not eligible,
        2 over a route's cap); d_rows64 f64 [n_vox, nS], the denoised rows before the float32 rounding, NaN where status != 0
        (amx_prep_noise_mppca_denoise_device); enqueued on `stream`"""
        self.ctx.check(lib().amx_prep_noise_mppca_denoise_device(self.ctx._h, self._h, c_vp(d_img), int(patch), c_vp(d_out or 0), c_vp(d_sigma or 0),
                                                                 c_vp(d_nsignal or 0), c_vp(d_mean or 0), c_vp(d_ratio or 0), c_vp(d_status or 0),
                                                                 c_vp(d_rows64 or 0), c_vp(stream or 0)))

    def sanitize(self, img, replace=None):
        """host image: -> number of NaN / Inf samples; with `replace` (a finite number) they are overwritten IN PLACE with float32(replace),
        np.nan_to_num(img, copy=False, nan=r, posinf=r, neginf=r) of core.py:156 (amx_prep_sanitize)"""
        buf = self._img_buffer(img)
        if replace is not None and not img.flags.writeable:
            raise ValueError('the image is sanitized in place and must be writeable')
        out = C.c_int64()
        self.ctx.check(lib().amx_prep_sanitize(self.ctx._h, self._h, _p(buf, c_fp), int(replace is not None), _replacement(replace, np.float32),
                                               C.byref(out)))
        return int(out.value)

    def sanitize_device(self, d_img, replace=None, stream=None):
        """device pointer (int) of the image's element buffer, enqueued on `stream`; the count: Context.sanitize_last()"""
        self.ctx.check(lib().amx_prep_sanitize_device(self.ctx._h, self._h, c_vp(d_img), int(replace is not None), _replacement(replace, np.float32),
                                                      c_vp(stream or 0)))

    def _raw_buffer(self, raw):
        """the image in its stored dtype as the flat element buffer the plan's strides refer to, counted in its own elements"""
        if raw.dtype not in RAW_DTYPES or raw.shape != self.shape or tuple(s // raw.itemsize for s in raw.strides) != self.strides \
                or any(s % raw.itemsize for s in raw.strides):
            raise ValueError('raw image does not match the plan (one of uint8 / int16 / uint16 / int32 / float32 / float64, shape, strides)')
        return np.lib.stride_tricks.as_strided(raw, shape=(self.extent,), strides=(raw.itemsize,))

    def ingest_device(self, d_raw, raw_dtype, d_img, scaling=None, replace=None, stream=None):
        """device pointers (ints): the image in its stored dtype (the plan's element strides) -> the float32 image of core.py:136, NaN / Inf
        scan and replacement included (amx_prep_ingest_device); enqueued on `stream`; the count: Context.sanitize_last().
        scaling: (slope, inter) of the NIfTI header or None; a layout that cannot be streamed is a ValueError"""
        slope, inter = (1.0, 0.0) if scaling is None else scaling
        self.ctx.check(lib().amx_prep_ingest_device(self.ctx._h, self._h, c_vp(d_raw), RAW_DTYPES[np.dtype(raw_dtype)], float(slope), float(inter),
                                                    int(replace is not None), _replacement(replace, np.float32), c_vp(d_img), c_vp(stream or 0)))

    def ingest(self, raw, scaling=None, replace=None):
        """host image in its stored dtype -> (float32 image in the same layout, number of NaN / Inf samples found) (amx_prep_ingest)"""
        buf = self._raw_buffer(raw)
        slope, inter = (1.0, 0.0) if scaling is None else scaling
        flat = np.empty(self.extent, dtype=np.float32)
        out = C.c_int64()
        self.ctx.check(lib().amx_prep_ingest(self.ctx._h, self._h, buf.ctypes.data_as(c_vp), RAW_DTYPES[raw.dtype], float(slope), float(inter),
                                             int(replace is not None), _replacement(replace, np.float32), _p(flat, c_fp), C.byref(out)))
        img = np.lib.stride_tricks.as_strided(flat, shape=self.shape, strides=tuple(4 * s for s in self.strides))
        return img, int(out.value)

    def corrected_device(self, lut, y_t, xiso_t, volume_t, mean_b0_t=None, b0_cols=(), stream=None):
        """RESULTS['DWI_corrected'] (core.py:488-498) in HBM: y f32 [n_vox, n_out], x_iso f64 [n_vox, n_iso] (rows in the plan's masked
        order) -> volume f32 [X, Y, Z, n_out], every element written once; mean_b0_t f32 [n_vox]: rescale by it (None: no rescaling);
        b0_cols: columns that keep y * mean_b0 (doKeepb0Intact).  Device tensors, enqueued on `stream` (amx_prep_corrected_device)"""
        import torch
        n = self.n_vox
        if y_t.dtype != torch.float32 or tuple(y_t.shape) != (n, self.n_out) or not y_t.is_contiguous():
            raise ValueError(f'y must be a contiguous float32 device tensor [{n}, {self.n_out}]')
        if xiso_t.dtype != torch.float64 or tuple(xiso_t.shape) != (n, lut.n_iso) or not xiso_t.is_contiguous():
            raise ValueError(f'x_iso must be a contiguous float64 device tensor [{n}, {lut.n_iso}]')
        if mean_b0_t is not None and (mean_b0_t.dtype != torch.float32 or tuple(mean_b0_t.shape) != (n,) or not mean_b0_t.is_contiguous()):
            raise ValueError(f'mean_b0 must be a contiguous float32 device tensor [{n}]')
        if volume_t.dtype != torch.float32 or tuple(volume_t.shape) != self.shape[:3] + (self.n_out,) or not volume_t.is_contiguous():
            raise ValueError('volume must be a contiguous float32 device tensor [X, Y, Z, n_out]')
        b0 = np.ascontiguousarray(b0_cols, dtype=np.int32).ravel()
        self.ctx.check(lib().amx_prep_corrected_device(self.ctx._h, self._h, lut._h, _dptr(y_t), _dptr(xiso_t), _dptr(mean_b0_t),
                                                       _p(b0, c_i32p) if len(b0) else None, len(b0), _dptr(volume_t), c_vp(stream or 0)))
        return volume_t

    def predicted_device(self, lut, x_t, volume_t, dirs_t=None, mean_b0_t=None, stream=None):
        """RESULTS['DWI_predicted'] in HBM: the coefficients x f64 [n_vox, n_atoms] (or NODDI's [n_vox, 3, n_atoms]) and the directions
        f64 [n_vox, 3] (None for SANDI), rows in the plan's masked order -> volume f32 [X, Y, Z, n_out] = float32(mean_b0 * A x), zeros
        outside the mask, every element written once; mean_b0_t f32 [n_vox]: rescale by it (None: no rescaling).  Device tensors,
        enqueued on `stream` (amx_prep_predicted_device)"""
        import torch
        n = self.n_vox
        stride, offset = _check_x(lut, x_t, dirs_t, n)
        if mean_b0_t is not None and (mean_b0_t.dtype != torch.float32 or tuple(mean_b0_t.shape) != (n,) or not mean_b0_t.is_contiguous()
                                      or mean_b0_t.device != x_t.device):
            raise ValueError(f'mean_b0 must be a contiguous float32 device tensor [{n}] on the device of x')
        if volume_t.dtype != torch.float32 or tuple(volume_t.shape) != self.shape[:3] + (self.n_out,) or not volume_t.is_contiguous() \
                or volume_t.device != x_t.device:
            raise ValueError('volume must be a contiguous float32 device tensor [X, Y, Z, n_out] on the device of x')
        self.ctx.check(lib().amx_prep_predicted_device(self.ctx._h, self._h, lut._h, _dptr(x_t), stride, offset, _dptr(dirs_t), _dptr(mean_b0_t),
                                                       _dptr(volume_t), c_vp(stream or 0)))
        return volume_t

    def scatter(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim == 1:
            v = v[:, None]
        if v.shape[0] != self.n_vox:
            raise ValueError('values must have one row per masked voxel')
        out = np.zeros(self.shape[:3] + (v.shape[1],), dtype=np.float32)
        self.ctx.check(lib().amx_prep_scatter(self.ctx._h, self._h, _p(v, c_dp), v.shape[1], _p(out, c_fp)))
        return out


PREP_ROUTES = ('refused', 'tile', 'long')      # amx_prep_route: out[0]


def prep_route(nS, n_out, n_b0, n_gidx, identity, direct, inplace):
    """the gather's route for a plan of these sizes, without a device (amx_prep_route)
    -> {'route': one of PREP_ROUTES, 'waves': wavefronts per workgroup, 'lds': bytes per workgroup, 'per_wave': words of one tile}"""
    out = np.zeros(4, dtype=np.int64)
    if lib().amx_prep_route(int(nS), int(n_out), int(n_b0), int(n_gidx), int(bool(identity)), int(bool(direct)), int(bool(inplace)),
                            _p(out, c_i64p)) != 0:
        raise ValueError('amx_prep_route: bad sizes')
    return {'route': PREP_ROUTES[int(out[0])], 'waves': int(out[1]), 'lds': int(out[2]), 'per_wave': int(out[3])}


MPPCA_SIDES = ('volumes', 'patch')             # amx_mppca_route: out[3]


def mppca_route(nS, patch, n_cols, dims):
    """the Marchenko-Pastur kernel's launch for a patch of n_cols masked columns in a volume of extents dims, without a device
    (amx_mppca_route; ValueError for a shape it refuses: patch not 3 or 5, nS > 512, an axis shorter than the patch)
    -> {'r', 'q', 'side': one of MPPCA_SIDES (what the Gram matrix is over), 'gram': its order, 'chunk': samples per staged chunk,
        'waves': wavefronts per patch, 'patches': per workgroup, 'lds': bytes per workgroup, 'eligible': 2 n_cols >= patch^3}"""
    out = np.zeros(10, dtype=np.int64)
    d = np.ascontiguousarray(dims, dtype=np.int64)
    if d.shape != (3,) or lib().amx_mppca_route(int(nS), int(patch), int(n_cols), _p(d, c_i64p), _p(out, c_i64p)) != 0:
        raise ValueError('amx_mppca_route: refused (patch 3 or 5, at most 512 volumes, no axis shorter than the patch)')
    return {'r': int(out[1]), 'q': int(out[2]), 'side': MPPCA_SIDES[int(out[3])], 'gram': int(out[4]), 'chunk': int(out[5]),
            'waves': int(out[6]), 'patches': int(out[7]), 'lds': int(out[8]), 'eligible': bool(out[9])}


def unring_route(n_a, n_b):
    """what the unringing kernels ask for a slice of n_a x n_b pixels, without a device (amx_unring_route; ValueError for an extent outside
    8 .. 256) -> {'tile': (rows, lines, depth) of the MFMA tile, 'pad': the extents rounded up to it, 'groups': workgroups per slice for
    the lines along a / along b, 'lds_dft', 'lds_shift': LDS bytes per workgroup, 'table_bytes', 'slice_bytes', 'chunk': slices per
    chunk, 'cap': the scratch cap in bytes}"""
    out = np.zeros(14, dtype=np.int64)
    if lib().amx_unring_route(int(n_a), int(n_b), _p(out, c_i64p)) != 0:
        raise ValueError('amx_unring_route: refused (each in-plane extent must be 8 to 256 pixels)')
    return {'tile': (int(out[1]), int(out[2]), int(out[3])), 'pad': (int(out[4]), int(out[5])), 'groups': (int(out[6]), int(out[7])),
            'lds_dft': int(out[8]), 'lds_shift': int(out[9]), 'table_bytes': int(out[10]), 'slice_bytes': int(out[11]),
            'chunk': int(out[12]), 'cap': int(out[13])}


def mppca_denoise_route(nS, patch, n_cols, dims):
    """the Marchenko-Pastur denoising kernel's launch for a patch of n_cols masked columns, without a device (amx_mppca_denoise_route;
    ValueError for what `mppca_route` refuses) -> {'r', 'q', 'side', 'waves', 'patches', 'per_patch': LDS bytes of a patch, 'lds': bytes per
    workgroup, 'capacity': eigenvectors of length r the kernel holds, 'cap': the most min(n_signal, r - n_signal) may be (0: no cap),
    'eligible'}"""
    out = np.zeros(11, dtype=np.int64)
    d = np.ascontiguousarray(dims, dtype=np.int64)
    if d.shape != (3,) or lib().amx_mppca_denoise_route(int(nS), int(patch), int(n_cols), _p(d, c_i64p), _p(out, c_i64p)) != 0:
        raise ValueError('amx_mppca_denoise_route: refused (patch 3 or 5, at most 512 volumes, no axis shorter than the patch)')
    return {'r': int(out[1]), 'q': int(out[2]), 'side': MPPCA_SIDES[int(out[3])], 'waves': int(out[4]), 'patches': int(out[5]),
            'per_patch': int(out[6]), 'lds': int(out[7]), 'capacity': int(out[8]), 'cap': int(out[9]), 'eligible': bool(out[10])}


NODDI_BUILDS = ('none', 'small', 'f32_8', 'f64_12', 'f64_nw', 'f32_nw', 'global', 'gram', 'gram_left', 'qr', 'big_all')      # NoddiBuild (csrc/amx_noddi_route.hpp)
NODDI_ROUTE_WORDS = ('seeds', 'global', 'gemm_ks', 'gemm_passes', 'gemm_window', 'gcert', 'repair', 'rescue', 'tile_in_lds', 'seeds2', 'gcert2', 'wide',
                     'third', 'min_items', 'seed2_max_atoms', 'seed2_trip_add', 'left2_second_half', 'left2_count', 'seed_occ2', 'seed2_occ2',
                     'seed_chunk', 'seed_waves', 'seed1_waves', 'seed2_waves', 's1', 's2', 's2_gram', 's3', 'n_launch', 'gemm', 'NR', 'gcert2_wide_lds')
NODDI_GEMMS = ('none', 'windows', '25_9', '25', '40')      # NoddiGemm


def noddi_route(nS, n_wm, n_dwi, ndirs, is_exvivo, n_vox, call_vox=0, lambda1=0.5, lambda2=1e-3):
    """which kernels a NODDI fit of n_vox voxels (a batch of a call of call_vox voxels; 0: the call itself) launches on a dictionary of this
    shape, every switch at its default, without a device (amx_noddi_route) -> the words of NODDI_ROUTE_WORDS (flags as bool, s1 / s2 / s3 as
    names of NODDI_BUILDS, gemm of NODDI_GEMMS), 'path' in the format of Context.last_path() and 'launches': [(kernel, wavefronts, LDS bytes, LDS bytes of its
    re-run pass)] in launch order"""
    out = np.zeros(96, dtype=np.int64)
    buf = C.create_string_buffer(2048)
    if lib().amx_noddi_route(int(nS), int(n_wm), int(n_dwi), int(ndirs), int(bool(is_exvivo)), int(n_vox), int(call_vox), float(lambda1),
                             float(lambda2), buf, 2048, _p(out, c_i64p)) != 0:
        raise ValueError('amx_noddi_route: bad sizes')
    rt = {k: int(v) for k, v in zip(NODDI_ROUTE_WORDS, out)}
    for k in ('seeds', 'global', 'gcert', 'repair', 'rescue', 'tile_in_lds', 'seeds2', 'gcert2', 'wide', 'third', 'left2_second_half', 'seed_occ2',
              'seed2_occ2', 's2_gram'):
        rt[k] = bool(rt[k])
    for k in ('s1', 's2', 's3'):
        rt[k] = NODDI_BUILDS[rt[k]]
    rt['gemm'] = NODDI_GEMMS[rt['gemm']]
    rt['path'] = buf.value.decode()
    names = rt['path'].split(' -> ')
    w = out[len(NODDI_ROUTE_WORDS):len(NODDI_ROUTE_WORDS) + 3 * rt['n_launch']].reshape(-1, 3)
    rt['launches'] = [(names[i], int(w[i, 0]), int(w[i, 1]), int(w[i, 2])) for i in range(rt['n_launch'])]
    return rt


# SmallFamily, SmallTables, SmallRefusal (csrc/amx_small_route.hpp); the switches of switches_mask, bit 0 first
SMALL_FAMILIES = ('none', 'fw_fused', 'fw_refill', 'lane', 'wave', 'sandi_rows', 'sandi_long_lane', 'sandi_long_wave', 'czb_fast', 'czb_gram', 'czb_qr',
                  'enet_big')
SMALL_TABLES = ('none', 'fw', 'sandi', 'sandi_long', 'czb')
SMALL_REFUSALS = ('none', 'sandi_long_ridge', 'pair_tile', 'lane_tile', 'sandi_long_operand', 'big_no_gram', 'big_vectors')
SMALL_SWITCHES = ('AMX_WAVE_PER_VOXEL', 'AMX_NO_REFILL', 'AMX_SANDI_ATOM_SPACE', 'AMX_FW_NO_FUSE')
SMALL_ROUTE_WORDS = ('family', 'N', 'NR', 'mfma', 'widen', 'chunk', 'blocks_chunk', 'tables', 'in_order', 'nSp', 'waves', 'lds', 'lds_list', 'refusal',
                     'n_launch')


def small_route(model, nS, n_atoms, ndirs, n_vox, lambda1=0.0, lambda2=1e-3, flags=0, f32=False, switches_mask=0):
    """which kernels a FreeWater (model 2), SANDI (3) or CylinderZeppelinBall (4) fit of n_vox voxels launches on a dictionary of this shape,
    without a device (amx_small_route) -> the words of SMALL_ROUTE_WORDS ('family', 'tables', 'refusal' as names of SMALL_FAMILIES /
    SMALL_TABLES / SMALL_REFUSALS, flags as bool), 'path' in the format of Context.last_path(), 'launches' (its kernels), 'status' (AMX_OK, or
    AMX_E_BADARG for a shape the fit refuses) and 'error' (the refusal's text)"""
    out = np.zeros(len(SMALL_ROUTE_WORDS), dtype=np.int64)
    buf = C.create_string_buffer(1024)
    if lib().amx_small_route(int(model), int(nS), int(n_atoms), int(ndirs), int(n_vox), float(lambda1), float(lambda2), int(flags), int(bool(f32)),
                             int(switches_mask), buf, 1024, _p(out, c_i64p)) != 0:
        raise ValueError('amx_small_route: bad arguments')
    rt = {k: int(v) for k, v in zip(SMALL_ROUTE_WORDS, out)}
    for k in ('mfma', 'widen', 'in_order'):
        rt[k] = bool(rt[k])
    rt['family'], rt['tables'], rt['refusal'] = SMALL_FAMILIES[rt['family']], SMALL_TABLES[rt['tables']], SMALL_REFUSALS[rt['refusal']]
    rt['path'], _, rt['error'] = buf.value.decode().partition('\n')
    rt['launches'] = rt['path'].split(' -> ') if rt['path'] else []
    rt['status'] = AMX_E_BADARG if rt['refusal'] != 'none' else AMX_OK
    return rt


def _replacement(replace, dtype):
    """the value handed to the library: `replace` rounded ONCE to the buffer's type (what numpy's assignment into the image does); 0 when
    nothing is to be replaced.  A value that is finite but overflows the type becomes Inf here and the library refuses it."""
    if replace is None:
        return 0.0
    with np.errstate(over='ignore'):
        return float(dtype(replace))


def sanitize_device(ctx, d_buf, count, replace=None, stream=None, f32=True):
    """`count` contiguous float32 (f32=True) | float64 elements at device pointer `d_buf` (int): count the NaN / Inf elements and, with
    `replace`, overwrite them (amx_sanitize_device[_f32]); enqueued on `stream`; the count: Context.sanitize_last()"""
    fn = lib().amx_sanitize_device_f32 if f32 else lib().amx_sanitize_device
    ctx.check(fn(ctx._h, c_vp(d_buf), int(count), int(replace is not None), _replacement(replace, np.float32 if f32 else np.float64),
                 c_vp(stream or 0)))


def sanitize(ctx, y, replace=None):
    """host float64 array (C-contiguous), IN PLACE when `replace` is given: -> number of NaN / Inf elements (amx_sanitize)"""
    if y.dtype != np.float64 or not y.flags.c_contiguous or (replace is not None and not y.flags.writeable):
        raise ValueError('y must be a C-contiguous (writeable) float64 array')
    out = C.c_int64()
    ctx.check(lib().amx_sanitize(ctx._h, _p(y, c_dp), y.size, int(replace is not None), _replacement(replace, np.float64), C.byref(out)))
    return int(out.value)


def debias_rows(ctx, S, b0_idx, snr):
    """S f32 | f64 [n, nS] -> E f64 [n, nS]: the exact minimiser of preproc.py's functional, row by row (amx_debias_rows[_f32])"""
    S = np.asarray(S)
    if S.ndim != 2:
        raise ValueError('S must be [n, nS]')
    f32 = S.dtype == np.float32
    S = np.ascontiguousarray(S, dtype=np.float32 if f32 else np.float64)
    b0 = np.ascontiguousarray(b0_idx, dtype=np.int32)
    E = np.empty(S.shape, dtype=np.float64)
    fn = lib().amx_debias_rows_f32 if f32 else lib().amx_debias_rows
    ctx.check(fn(ctx._h, _p(S, c_fp if f32 else c_dp), S.shape[0], S.shape[1], _p(b0, c_i32p), len(b0), float(snr), _p(E, c_dp)))
    return E


def noise_b0_rows_device(ctx, d_S, n, nS, b0_idx, d_mean=None, d_sd=None, d_ratio=None, stream=None, f32=False):
    """device pointers (ints): rows S f64 | f32 (f32=True) [n, nS] -> mean, sd (ddof = 1) and mean / sd of the samples b0_idx (host, in
    that order), f64 [n] each, NaN where a row is not eligible; any of the three may be None, not all (amx_noise_b0_rows_device[_f32])"""
    b0 = np.ascontiguousarray(b0_idx, dtype=np.int32).ravel()
    fn = lib().amx_noise_b0_rows_device_f32 if f32 else lib().amx_noise_b0_rows_device
    ctx.check(fn(ctx._h, c_vp(d_S or 0), int(n), int(nS), _p(b0, c_i32p), len(b0), c_vp(d_mean or 0), c_vp(d_sd or 0), c_vp(d_ratio or 0),
                 c_vp(stream or 0)))


def nanmedian_device(ctx, d_v, n, d_out, d_count, stream=None):
    """device pointers (ints): v f64 [n] -> out f64 [2] = the lower and upper middle of its non-NaN values, count int64 [1] = how many
    there are (0: both NaN); numpy's nanmedian is (out[0] + out[1]) / 2 (amx_nanmedian_device); enqueued on `stream`"""
    ctx.check(lib().amx_nanmedian_device(ctx._h, c_vp(d_v or 0), int(n), c_vp(d_out or 0), c_vp(d_count or 0), c_vp(stream or 0)))


def lut_resample(ctx, lm, ylm_out, idx_out, nS):
    """lm f32[..., n_sh] -> f32[..., nS] with ones outside idx_out (resample_kernel, lut.pyx:274-311, batched)"""
    lm = np.ascontiguousarray(lm, dtype=np.float32)
    y = np.ascontiguousarray(ylm_out, dtype=np.float32)
    idx = np.ascontiguousarray(idx_out, dtype=np.int32)
    if y.ndim != 2 or lm.shape[-1] != y.shape[1] or idx.shape != (y.shape[0],):
        raise ValueError('Outdated LUT. Call "generate_kernels( regenerate=True )" to update the LUT')   # lut.pyx:301
    rows = int(np.prod(lm.shape[:-1], dtype=np.int64))
    out = np.empty(lm.shape[:-1] + (int(nS),), dtype=np.float32)
    ctx.check(lib().amx_lut_resample(ctx._h, _p(lm, c_fp), rows, lm.shape[-1], _p(y, c_fp), _p(idx, c_i32p),
                                     y.shape[0], int(nS), _p(out, c_fp)))
    return out


LUT_ROUTES = ('refused', 'tile', 'lds', 'generic')      # LUT_ROUTE_* (csrc/amx_lut_route.hpp)


def lut_route(n_sh, n_out, fused=False):
    """which kernel the resampling GEMM launches for K = n_sh reduction indices and n_out volumes (fused: lut_rotate_resample), without a
    device (amx_lut_route) -> {'route': one of LUT_ROUTES, 'kh2': compile-time half-length 23 / 46 / 64, 'lds': dynamic LDS bytes}"""
    out = np.zeros(3, dtype=np.int64)
    if lib().amx_lut_route(int(n_sh), int(n_out), int(bool(fused)), _p(out, c_i64p)) != 0:
        raise ValueError('amx_lut_route: bad sizes')
    return {'route': LUT_ROUTES[int(out[0])], 'kh2': int(out[1]), 'lds': int(out[2])}


def lut_rotate_resample(ctx, zonal, ylm_rot, ylm_out, idx_out, nS):
    """zonal f32[n_atoms, n_shells * nSH] (const * Klm[idx_m0] per shell), ylm_rot f32[ndirs, nSH] -> f32[n_atoms, ndirs, nS]:
    rotate_kernel + resample_kernel of lut.pyx:227-311 in one GEMM whose left operand is formed on the fly"""
    z = np.ascontiguousarray(zonal, dtype=np.float32)
    r = np.ascontiguousarray(ylm_rot, dtype=np.float32)
    y = np.ascontiguousarray(ylm_out, dtype=np.float32)
    idx = np.ascontiguousarray(idx_out, dtype=np.int32)
    if z.ndim != 2 or r.ndim != 2 or y.ndim != 2 or z.shape[1] % r.shape[1] or y.shape[1] != z.shape[1] or idx.shape != (y.shape[0],):
        raise ValueError('Outdated LUT. Call "generate_kernels( regenerate=True )" to update the LUT')
    out = np.empty((z.shape[0], r.shape[0], int(nS)), dtype=np.float32)
    ctx.check(lib().amx_lut_rotate_resample(ctx._h, _p(z, c_fp), z.shape[0], _p(r, c_fp), r.shape[0], r.shape[1],
                                            z.shape[1] // r.shape[1], _p(y, c_fp), _p(idx, c_i32p), y.shape[0], int(nS), _p(out, c_fp)))
    return out
