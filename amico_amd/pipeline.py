"""Device-resident chain of the per-voxel steps: raw float32 image (in HBM) -> float32 map volumes (in HBM).

    amx_prep_ingest_device              the image in its stored dtype -> float32, scan included (optional: raw_dtype / scaling) core.py:136
    amx_prep_sanitize_device            NaN / Inf samples of the image replaced (optional: replace_bad_voxels) core.py:152-156
    amx_prep_debias_device              Rician debias in place (optional: debias_snr)                     core.py:201-206, preproc.py:23-36
    amx_prep_gather_directions_device   b0 normalisation (+ merge / shell average), mask gather, clip     core.py:209-268, 451-452
                                        AND the principal directions (log-linear tensor fit)            core.py:428-436, 456-458
    amx_sanitize_device_f32             NaN / Inf values of y replaced (optional: replace_bad_voxels)     core.py:270-274
    amx_noddi_fit_device        NNLS -> LASSO -> NNLS, maps                                        models.pyx:816-991
      | amx_freewater_fit_device  lasso, maps (+ the isotropic coefficients, AMX_F_FW_ISO)           models.pyx:1168-1286
    amx_prep_scatter_device     maps / directions into float32 volumes                             core.py:472-498
    amx_prep_corrected_device   FreeWater: the corrected DWI volume (optional: corrected)          models.pyx:1264-1274, core.py:488-498

tensor_maps=True (Evaluation's doSaveTensorMaps) replaces the fused kernel by amx_prep_gather_device + amx_dti_fit_device_f32, which also
leaves the tensor's eigenvalues and FA, MD, AD, RD; they are scattered into `dti_evals` / `dti_maps`.  FreeWater then makes the
corrected rows in HBM (amx_freewater_corrected_device) and fits the tensor again on them -> `dti_maps_corrected` / `dti_evals_corrected`.

Everything is enqueued on one HIP stream; the only host synchronisation is `amx_sync_status` at the end.  torch is
used for device buffers only.  `amico_amd.core.Evaluation` is the host-array (numpy in / numpy out) face of the
same chain.
"""
import numpy as np

from . import _capi, dti as _dti, prep as _prep
from .models import get_context


class _VolumePipeline:
    """what the model pipelines share: the plan, the buffers of the prepared signals and the directions, the chain up to the fit
    (scan, debias, gather + directions, scan of y) and run()"""

    def _setup(self, scheme, img_like, mask, do_normalize, b0_min_signal, device, fused, debias_snr, replace_bad_voxels,
               raw_dtype=None, scaling=None, tensor_maps=False):
        import torch
        # tensor_maps: the tensor pass also writes its eigenvalues and FA, MD, AD, RD (amx_dti_fit_device_f32).  The fused gather has no
        # such variant, so the chain is gather -> tensor pass whatever `fused` says: the OLS fit no longer rides on the gather
        self.tensor_maps = bool(tensor_maps)
        # raw_dtype: run() is given the image in that stored dtype (the plan's geometry and element strides) and starts with the ingest
        # kernel, which makes the float32 image `self.img` and does the scan of the image in the same pass; a scaling alone means float32
        self.scaling = _prep.check_scaling(scaling)
        if raw_dtype is None and (self.scaling is not None or img_like.dtype != np.float32):
            raw_dtype = img_like.dtype if img_like.dtype in _capi.RAW_DTYPES else np.float32
        self.raw_dtype = None if raw_dtype is None else np.dtype(raw_dtype)
        if self.raw_dtype is not None and self.raw_dtype not in _capi.RAW_DTYPES:
            raise ValueError('raw_dtype must be one of uint8, int16, uint16, int32, float32, float64')
        if self.raw_dtype == np.float32 and self.scaling is None:
            self.raw_dtype = None          # float32 as it is: the chain of today, nothing more is launched
        self.fused = bool(fused)           # False: gather, then the tensor fit as its own pass over y (the round-4 chain; A/B)
        self.torch = torch
        self.ctx = get_context()
        self.dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        self.scheme = scheme
        self.prep = _prep.SignalPreparation(scheme, img_like, mask, do_normalize=do_normalize,
                                            b0_min_signal=b0_min_signal, ctx=self.ctx, debias_snr=debias_snr,
                                            replace_bad_voxels=replace_bad_voxels)
        self.replace_bad_voxels = self.prep.replace_bad_voxels
        self.bad_samples = self.bad_samples_preprocessed = None
        if b0_min_signal != 0.0:
            raise NotImplementedError('b0_min_signal needs the whole-volume b0 mean on the host: use Evaluation')
        self.tensor = _dti.TensorDirections.from_scheme(scheme, ctx=self.ctx)
        self.img = None
        if self.raw_dtype is not None:
            self.img = torch.empty(self.prep._plan.extent, dtype=torch.float32, device=self.dev)

    def _buffers(self, n_maps):
        torch = self.torch
        n = self.prep.n_vox
        self.n_vox = n
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.y = torch.empty((n, self.scheme.nS), dtype=torch.float32, device=self.dev)      # float32 like the image (core.py:136)
        self.dirs = torch.empty((n, 3), **f64)
        self.est = torch.empty((n, n_maps), **f64)
        self.mean_b0 = torch.empty(n, dtype=torch.float32, device=self.dev)
        self.maps = torch.empty(self.shape + (n_maps,), dtype=torch.float32, device=self.dev)
        self.dirs_vol = torch.empty(self.shape + (3,), dtype=torch.float32, device=self.dev)
        self.dti_maps = self.dti_evals = None
        if self.tensor_maps:
            self._evals, self._scalars = torch.empty((n, 3), **f64), torch.empty((n, 4), **f64)
            self.dti_evals = torch.empty(self.shape + (3,), dtype=torch.float32, device=self.dev)
            self.dti_maps = torch.empty(self.shape + (4,), dtype=torch.float32, device=self.dev)      # FA, MD, AD, RD

    def _enqueue_signals(self, d_img, stream):
        """image -> y, mean_b0, dirs (everything ahead of the model fit)"""
        c, p = self.ctx, self.prep._plan
        r = self.replace_bad_voxels
        if self.raw_dtype is not None:
            # core.py:136 and the scan of the image in one kernel; everything below reads the float32 image it leaves in self.img
            p.ingest_device(d_img.data_ptr(), self.raw_dtype, self.img.data_ptr(), self.scaling, r, stream)
            d_img = self.img
        elif r is not None:
            p.sanitize_device(d_img.data_ptr(), r, stream)
        if self.prep.debias_snr is not None:
            p.debias_device(d_img.data_ptr(), self.prep.debias_snr, stream)
        if self.tensor_maps:
            p.gather_device(d_img.data_ptr(), self.y.data_ptr(), self.mean_b0.data_ptr(), self.prep.do_normalize, 0.0, stream)
            if r is not None:
                _capi.sanitize_device(c, self.y.data_ptr(), self.y.numel(), r, stream)
            self.tensor.fit_device(self.y.data_ptr(), self.n_vox, self.dirs.data_ptr(), stream, f32=True,
                                   d_evals=self._evals.data_ptr(), d_scalars=self._scalars.data_ptr())
            return
        if self.fused:
            # one pass over the image: the tensor fit rides on the gather's LDS tile
            p.gather_directions_device(self.tensor._dti, d_img.data_ptr(), self.y.data_ptr(), self.mean_b0.data_ptr(), self.dirs.data_ptr(),
                                       self.prep.do_normalize, 0.0, stream)
        else:
            p.gather_device(d_img.data_ptr(), self.y.data_ptr(), self.mean_b0.data_ptr(), self.prep.do_normalize, 0.0, stream)
            if r is not None:
                _capi.sanitize_device(c, self.y.data_ptr(), self.y.numel(), r, stream)
            self.tensor.fit_device(self.y.data_ptr(), self.n_vox, self.dirs.data_ptr(), stream, f32=True)
        if r is not None and self.fused:
            _capi.sanitize_device(c, self.y.data_ptr(), self.y.numel(), r, stream)

    def _enqueue_scatter(self, stream):
        p = self.prep._plan
        p.scatter_device(self.est.data_ptr(), self.est.shape[1], self.maps.data_ptr(), stream)
        p.scatter_device(self.dirs.data_ptr(), 3, self.dirs_vol.data_ptr(), stream)
        if self.tensor_maps:
            p.scatter_device(self._evals.data_ptr(), 3, self.dti_evals.data_ptr(), stream)
            p.scatter_device(self._scalars.data_ptr(), 4, self.dti_maps.data_ptr(), stream)

    def run(self, d_img, stream=None):
        self.enqueue(d_img, stream)
        self.ctx.sync(stream)
        if self.replace_bad_voxels is not None:
            # the chain's two scans are the last two sanitize calls of the context: image first, y second
            self.bad_samples, self.bad_samples_preprocessed = self.ctx.sanitize_previous(), self.ctx.sanitize_last()
        elif self.raw_dtype is not None:
            self.bad_samples = self.ctx.sanitize_last()       # the ingest kernel counts whether or not it replaces
        return self.maps, self.dirs_vol


class NoddiVolumePipeline(_VolumePipeline):
    def __init__(self, scheme, img_like, mask, kernels, htable, lambda1=0.5, lambda2=1e-3, do_normalize=True,
                 b0_min_signal=0.0, device=None, fused=True, debias_snr=None, replace_bad_voxels=None, raw_dtype=None, scaling=None,
                 tensor_maps=False):
        """tensor_maps=True: run() also leaves `dti_maps` [X, Y, Z, 4] (FA, MD, AD, RD) and `dti_evals` [X, Y, Z, 3] of the tensor fit
        in HBM (float32, zero outside the mask); the chain is then gather -> tensor pass, as with fused=False.
        raw_dtype / scaling: run() takes the image as it is stored (uint8, int16, uint16, int32, float32 or float64 elements in the
        layout of `img_like`, which must be C or Fortran ordered) plus the NIfTI header's (slope, inter); the chain then starts with the
        kernel that makes the float32 image in HBM (amx_prep_ingest_device) and counts its NaN / Inf samples into `bad_samples`.
        replace_bad_voxels: None leaves the chain as it is (no scan; a NaN in the image is the caller's).  A finite number enqueues
        the scan of the image ahead of everything else and the scan of y behind the gather, both replacing what they find, on
        the same stream and without a host wait; run() then leaves the two counts in `bad_samples` (image) and
        `bad_samples_preprocessed` (y).  With fused=True the gather computes the directions in the same kernel as y, so the
        directions of a voxel whose y is replaced afterwards come from the unreplaced values (fused=False fits them from the replaced y)."""
        self._setup(scheme, img_like, mask, do_normalize, b0_min_signal, device, fused, debias_snr, replace_bad_voxels, raw_dtype, scaling,
                    tensor_maps)
        self.lut = _capi.upload_noddi(self.ctx, kernels, htable, scheme.dwi_idx)
        self.lambda1, self.lambda2 = float(lambda1), float(lambda2)
        self.shape = tuple(img_like.shape[:3])
        self._buffers(3)

    def enqueue(self, d_img, stream=None):
        """d_img: torch float32 tensor holding the image's element buffer (same strides as `img_like`) -- with raw_dtype set, a tensor
        holding the elements of that dtype instead (any torch dtype: only its memory is used), which is left as it is; with debias_snr
        set the caller's d_img is OVERWRITTEN first: debiased where mask != 0, zero elsewhere; with replace_bad_voxels set its
        NaN / Inf samples are overwritten before that"""
        self._enqueue_signals(d_img, stream)
        _capi._fit_device(_capi.FIT['noddi'], self.ctx, self.lut, self.y, self.dirs, self.lambda1, self.lambda2, (3,), {}, stream, False, False,
                          into=self.est)
        self._enqueue_scatter(stream)


class FreeWaterVolumePipeline(_VolumePipeline):
    def __init__(self, scheme, img_like, mask, kernels, htable, lambda1=0.0, lambda2=1e-3, do_normalize=True,
                 b0_min_signal=0.0, device=None, fused=True, debias_snr=None, replace_bad_voxels=None,
                 corrected=False, keep_b0=False, is_mouse=False, raw_dtype=None, scaling=None, tensor_maps=False):
        """The chain of NoddiVolumePipeline (same arguments, same meaning) with the Free-Water fit: leaves `maps` [X, Y, Z, 2 | 4 (Mouse)]
        and `dirs_vol` in HBM.  corrected=True (doSaveCorrectedDWI): also `corrected` [X, Y, Z, nS], the free-water-corrected DWI of
        core.py:488-498 -- rescaled by the b0 mean when do_normalize is set; keep_b0=True (doKeepb0Intact) leaves its b0 volumes
        as they were.  The fit stays on its fast kernel: it hands over the isotropic coefficients only (AMX_F_FW_ISO).
        tensor_maps=True: as for NoddiVolumePipeline, and `dti_maps_corrected` / `dti_evals_corrected`: the same tensor fit on the
        corrected rows, which are made in HBM from the same isotropic coefficients (`corrected` need not be set)."""
        self._setup(scheme, img_like, mask, do_normalize, b0_min_signal, device, fused, debias_snr, replace_bad_voxels, raw_dtype, scaling,
                    tensor_maps)
        self.lut = _capi.upload_freewater(self.ctx, kernels, htable)
        self.lambda1, self.lambda2 = float(lambda1), float(lambda2)
        self.is_mouse = bool(is_mouse)
        self.shape = tuple(img_like.shape[:3])
        self._buffers(4 if self.is_mouse else 2)
        torch = self.torch
        self.want_corrected = bool(corrected)
        self.b0_cols = np.asarray(scheme.b0_idx, dtype=np.int32) if (keep_b0 and scheme.b0_count > 0) else np.zeros(0, dtype=np.int32)
        self.x_iso = self.corrected = self.dti_maps_corrected = self.dti_evals_corrected = None
        if self.want_corrected or self.tensor_maps:
            self.x_iso = torch.empty((self.n_vox, self.lut.n_iso), dtype=torch.float64, device=self.dev)
        if self.want_corrected:
            self.corrected = torch.empty(self.shape + (scheme.nS,), dtype=torch.float32, device=self.dev)
        if self.tensor_maps:
            f64 = dict(dtype=torch.float64, device=self.dev)
            self._evals_c, self._scalars_c = torch.empty((self.n_vox, 3), **f64), torch.empty((self.n_vox, 4), **f64)
            self._y_c = torch.empty((self.n_vox, scheme.nS), **f64)             # the corrected rows: they stay in HBM
            self.dti_evals_corrected = torch.empty(self.shape + (3,), dtype=torch.float32, device=self.dev)
            self.dti_maps_corrected = torch.empty(self.shape + (4,), dtype=torch.float32, device=self.dev)

    def enqueue(self, d_img, stream=None):
        """d_img: as for NoddiVolumePipeline.enqueue"""
        self._enqueue_signals(d_img, stream)
        _capi._fit_device(_capi.FIT['freewater'], self.ctx, self.lut, self.y, self.dirs, self.lambda1, self.lambda2, (int(self.is_mouse),), {},
                          stream, False, self.x_iso if self.x_iso is not None else False, into=self.est)
        self._enqueue_scatter(stream)
        if self.want_corrected:
            rescale = self.prep.do_normalize and self.scheme.b0_count > 0
            self.prep._plan.corrected_device(self.lut, self.y, self.x_iso, self.corrected, self.mean_b0 if rescale else None, self.b0_cols, stream)
        if self.tensor_maps:
            p = self.prep._plan
            _capi.freewater_corrected_device(self.ctx, self.lut, self.y, self.x_iso, stream, into=self._y_c)
            self.tensor.fit_device(self._y_c.data_ptr(), self.n_vox, None, stream, d_evals=self._evals_c.data_ptr(),
                                   d_scalars=self._scalars_c.data_ptr())
            p.scatter_device(self._evals_c.data_ptr(), 3, self.dti_evals_corrected.data_ptr(), stream)
            p.scatter_device(self._scalars_c.data_ptr(), 4, self.dti_maps_corrected.data_ptr(), stream)
