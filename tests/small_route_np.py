"""The cases of tests/golden/small_routes.json -- FreeWater, SANDI and CylinderZeppelinBall fits on both sides of every branch of
csrc/amx_small_route.hpp -- and the synthetic dictionaries and signals the GPU test fits them on (tests/test_gpu_small_route.py).
The route depends on the dictionary's shape alone, so the dictionaries are the cheapest amico_amd.synthetic makes at that shape:
five LUT orientations, one b0 volume and nS - 1 volumes on one shell (SANDI: nS - 1 shells after the directional average)."""
import functools

import numpy as np

N_VOX = 2048
N_ORI = 5
F_RMSE, F_CORRECTED = 1, 8              # AMX_F_* (include/amico_amd.h)
MODELS = {2: 'freewater', 3: 'sandi', 4: 'czb'}


def _c(model, n_atoms, nS, lam2=1e-3, flags=0, f32=False, mouse=False):
    return dict(model=model, n_atoms=n_atoms, nS=nS, lam1=0.0, lam2=lam2, flags=flags, f32=f32, mouse=mouse, n=N_VOX, ndirs=1 if model == 3 else N_ORI)


FW = ([_c(2, 11, nS, f32=f) for nS in (63, 64, 96, 97) for f in (False, True)] +              # the fuse, mfma and widen edges
      [_c(2, 12, 65, mouse=True), _c(2, 11, 227), _c(2, 11, 228),                             # ... the refill kernel's LDS bound
       _c(2, 11, 65, flags=F_RMSE), _c(2, 11, 65, flags=F_CORRECTED), _c(2, 13, 65), _c(2, 16, 65),
       _c(2, 11, 65, lam2=9.9e-6), _c(2, 11, 65, lam2=9.9e-10),
       _c(2, 17, 128), _c(2, 17, 129), _c(2, 17, 256), _c(2, 17, 257), _c(2, 64, 512), _c(2, 65, 65)])
SANDI = ([_c(3, 15, 6, lam2=l) for l in (1e-3, 9.9e-6, 9.9e-10)] +
         [_c(3, 12, 6), _c(3, 13, 6), _c(3, 16, 6), _c(3, 15, 7), _c(3, 17, 64), _c(3, 17, 65), _c(3, 15, 128), _c(3, 15, 129)] +
         [_c(3, a, 129) for a in (12, 13, 16, 17)] +
         [_c(3, 15, 129, f32=True), _c(3, 15, 129, lam2=9.9e-10),                             # ... the refusal
          _c(3, 65, 6), _c(3, 65, 129), _c(3, 15, 6, f32=True), _c(3, 17, 64, f32=True)])
CZB = ([_c(4, 26, nS) for nS in (100, 101, 160, 161)] +
       [_c(4, 26, 100, lam2=l) for l in (4.0, 1e-2, 9.9e-3, 1e-6, 9e-7)] +
       [_c(4, 26, 100, flags=F_RMSE), _c(4, 32, 100), _c(4, 33, 100), _c(4, 33, 129), _c(4, 33, 257), _c(4, 65, 100)] +
       # (beyond the issue's list: the fast route's own 100 / 101 and 160 / 161 edges need the strong ridge)
       [_c(4, 26, nS, lam2=4.0) for nS in (101, 160, 161)])
CASES = FW + SANDI + CZB


@functools.lru_cache(maxsize=None)
def orientations():
    from amico_amd import synthetic as S
    dirs = S.fibonacci_hemisphere(N_ORI)
    return dirs, S.build_htable(dirs)


def _rotated(n, nS, lo, hi):
    """n atoms of an axially symmetric compartment on the N_ORI orientations, float32 [n, N_ORI, nS]"""
    from amico_amd import synthetic as S
    sch = S.make_scheme(1, ((1000.0, nS - 1),), seed=3)
    return sch, S.freewater_kernels(sch, orientations()[0], d_perps=np.linspace(lo, hi, n) * 1e-3, d_isos=(2.5e-3, 1.5e-3))


@functools.lru_cache(maxsize=None)
def dictionary(model, n_atoms, nS, mouse=False):
    """(upload(ctx) -> Lut, A float64 [nS, n_atoms] of orientation 0)"""
    from amico_amd import _capi, synthetic as S
    ht = orientations()[1]
    if model == 2:
        n_iso = 2 if mouse else 1
        _, K = _rotated(n_atoms - n_iso, nS, 0.1, 1.0)
        K = dict(K, CSF=K['CSF'][:n_iso])
        A = np.concatenate([K['D'][:, 0], K['CSF']], axis=0).astype(np.float64).T
        return (lambda ctx: _capi.upload_freewater(ctx, K, ht)), A
    if model == 3:
        sch = S.directional_average_scheme(S.make_sandi_scheme(bvals=tuple(np.linspace(500.0, 8000.0, nS - 1)), ndir_per_shell=1, n_b0=1))
        a = n_atoms // 3
        K, Rs, d_in, d_isos = S.sandi_kernels(sch, Rs=np.linspace(1.0, 12.0, a) * 1e-6, d_in=np.linspace(0.25, 3.0, a) * 1e-3,
                                              d_isos=np.linspace(0.25, 3.0, n_atoms - 2 * a) * 1e-3)
        return (lambda ctx: _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)), np.ascontiguousarray(K['signal'], dtype=np.float64)
    n_perp = 4
    n_rs = n_atoms - n_perp - 1
    _, Kr = _rotated(n_rs, nS, 0.0, 0.08)           # (cylinders: nearly no diffusion across the axis)
    _, Kh = _rotated(n_perp, nS, 0.17, 1.19)
    K = {'model': 'CylinderZeppelinBall', 'wmr': Kr['D'], 'wmh': Kh['D'], 'iso': Kr['CSF'][:1]}
    Rs = np.linspace(0.5, 8.0, n_rs) * 1e-6
    A = np.concatenate([K['wmr'][:, 0], K['wmh'][:, 0], K['iso']], axis=0).astype(np.float64).T
    return (lambda ctx: _capi.upload_czb(ctx, K, Rs, ht)), A


def signals(A, n=N_VOX, seed=0):
    """(y [n, nS], dirs [n, 3]): sparse non-negative mixtures of the atoms of orientation 0 with a little noise, every voxel along that
    orientation"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, A.shape[1])) * (rng.uniform(size=(n, A.shape[1])) < 0.2)
    y = x @ A.T
    y = y / np.maximum(y.max(axis=1, keepdims=True), 1e-3) + 0.01 * rng.standard_normal(y.shape)
    return np.ascontiguousarray(np.abs(y)), np.ascontiguousarray(np.tile(orientations()[0][0], (n, 1)))


def fit(ctx, lut, c, y_t, d_t):
    """the device fit of case c -> (status, message): 0, or AMX_E_BADARG with the library's text"""
    from amico_amd import _capi
    want = dict(rmse=bool(c['flags'] & F_RMSE))
    try:
        if c['model'] == 2:
            _capi.freewater_fit_device(ctx, lut, y_t, d_t, c['lam1'], c['lam2'], c['mouse'], corrected=bool(c['flags'] & F_CORRECTED), **want)
        elif c['model'] == 3:
            _capi.sandi_fit_device(ctx, lut, y_t, c['lam1'], c['lam2'], **want)
        else:
            _capi.czb_fit_device(ctx, lut, y_t, d_t, c['lam1'], c['lam2'], **want)
        ctx.sync()
    except ValueError as e:
        return _capi.AMX_E_BADARG, str(e)
    return _capi.AMX_OK, ''
