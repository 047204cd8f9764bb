"""The wild bootstrap on the GPU (include/amico_amd.h: amx_bootstrap_*; amico_amd/bootstrap.py): the resample and the moment kernels bit
for bit against the numpy restatement of tests/bootstrap_np.py; the driver as the composition of its public parts, bit for bit; one leg
against the CPU oracle; the statistic's sanity; Evaluation's 'bootstrap_samples' / 'bootstrap_seed'.
Dictionaries and signals follow the recipe of tests/test_gpu_predicted.py (rebuilt here: nothing is imported from a test module)."""
import functools
import os

import numpy as np
import pytest

import bootstrap_np as B

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 65, 1037)          # one voxel, a wavefront less one, a wavefront and one, several workgroups and a remainder
VOLUMES = (6, 65, 99)
SEEDS = (0, 2 ** 63 + 5)
TOL, CAP, SHARE = 1e-6, 1e-4, 0.998       # what tests/test_gpu_parity.py holds a single NODDI fit to


@functools.lru_cache(maxsize=None)
def _htable():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'htable500.npz'), allow_pickle=False))


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------ 1. the resample kernel, bit for bit
@functools.lru_cache(maxsize=None)
def _resample_case(nS, dtype):
    """signals and predictions of the largest count: row 0 (and every 7th) has residuals larger than the prediction, so the mirrored
    samples are negative and the clip fires; row 2 has a NaN in the prediction.  Shared, not modified."""
    rng = np.random.default_rng(100 + nS)
    n = COUNTS[-1]
    ye = rng.uniform(0.05, 1.0, (n, nS))
    y = ye + rng.normal(scale=0.03, size=ye.shape)
    y[::7] = ye[::7] * rng.uniform(2.1, 3.0, (len(ye[::7]), nS))
    y = np.abs(y).astype(dtype)
    ye[2, nS // 2] = np.nan
    y.setflags(write=False)
    ye.setflags(write=False)
    return y, ye


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('nS', VOLUMES)
def test_resample_kernel_equals_the_restatement(nS, dtype):
    import torch
    from amico_amd import _capi, get_context
    y, ye = _resample_case(nS, dtype)
    ctx = get_context()
    clipped = 0
    for n in COUNTS:
        yt, et = torch.from_numpy(y[:n].copy()).cuda(), torch.from_numpy(ye[:n].copy()).cuda()
        yb = torch.empty_like(yt)
        for first in (0, 12345):
            for b in (0, 1, 97):
                for seed in SEEDS:
                    yb.fill_(-7.0)
                    got = _capi.bootstrap_resample_device(ctx, yt, et, seed, b, first, into=yb)
                    ctx.sync()
                    assert got is yb
                    got = got.cpu().numpy()
                    exp = B.resample(y[:n], ye[:n], seed, b, first)
                    assert got.dtype == dtype and _same(got, exp), (n, nS, first, b, seed, int((got != exp).sum()))
                    clipped += int(((got == 0) & (B.signs(seed, b, first, n, nS) < 0)).sum())
        if n > 2:
            assert np.isnan(got[2, nS // 2]) and np.isnan(got).sum() == 1
    assert clipped > 0
    # the inputs were not written
    assert _same(yt.cpu().numpy(), y) and _same(et.cpu().numpy(), ye)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_resample_kernel_on_pointers_that_are_not_16_byte_aligned(dtype):
    """buffers that start one element into an allocation: every element takes the one-by-one walk"""
    import torch
    from amico_amd import _capi, get_context
    nS = 65
    y, ye = _resample_case(nS, dtype)
    ctx = get_context()
    for n in (1, 65, 1037):
        def shifted(a):
            buf = torch.empty(a.size + 1, dtype=torch.float32 if a.dtype == np.float32 else torch.float64, device='cuda')
            view = buf[1:].view(a.shape)
            view.copy_(torch.from_numpy(a.copy()))
            return view
        yt, et = shifted(y[:n]), shifted(ye[:n])
        yb = shifted(np.full((n, nS), -7.0, dtype))
        assert yt.data_ptr() % 16 and et.data_ptr() % 16 and yb.data_ptr() % 16 and yt.is_contiguous()
        _capi.bootstrap_resample_device(ctx, yt, et, 7, 3, 11, into=yb)
        ctx.sync()
        assert _same(yb.cpu().numpy(), B.resample(y[:n], ye[:n], 7, 3, 11))


def test_resample_kernel_beyond_two_to_the_31_samples():
    """33.1 million voxels x 65 float32 volumes, 2.15e9 samples: constant signals (y = 0.25, y_est = 0.75, so a replicate sample is
    0.25 or 1.25 by its sign); windows at the start, across sample 2^31 and at the end are compared with the restatement"""
    import torch
    from amico_amd import _capi, get_context
    nS, n = 65, 33_100_000
    assert n * nS > 2 ** 31 + 2 ** 20
    ctx = get_context()
    yt = torch.full((n, nS), 0.25, dtype=torch.float32, device='cuda')
    et = torch.full((n, nS), 0.75, dtype=torch.float64, device='cuda')
    yb = torch.full((n, nS), -7.0, dtype=torch.float32, device='cuda')
    _capi.bootstrap_resample_device(ctx, yt, et, 5, 2, 0, into=yb)
    ctx.sync()
    v31 = 2 ** 31 // nS
    for lo in (0, v31 - 1000, n - 2001):
        got = yb[lo:lo + 2001].cpu().numpy()
        exp = B.resample(np.full((2001, nS), 0.25, np.float32), np.full((2001, nS), 0.75), 5, 2, lo)
        assert _same(got, exp), lo
        assert set(np.unique(got)) == {0.25, 1.25}
    # no sample was left out anywhere: every value is one of the two
    assert bool(((yb == 0.25) | (yb == 1.25)).all())


# ------------------------------------------------------------------ 2. the moments, bit for bit
@pytest.mark.parametrize('k', [2, 3, 4])
def test_moments_equal_the_restatement(k):
    import torch
    from amico_amd import _capi, get_context
    ctx = get_context()
    rng = np.random.default_rng(k)
    count = 5
    for n in COUNTS:
        maps = [rng.uniform(0.0, 1.0, (n, k)) * 10.0 ** rng.integers(-3, 3) for _ in range(count)]
        maps[2][n // 2, k - 1] = np.nan
        mean = torch.full((n, k), -7.0, dtype=torch.float64, device='cuda')      # (no memset needed: t = 1 writes both)
        m2 = torch.full((n, k), np.nan, dtype=torch.float64, device='cuda')
        for t, m in enumerate(maps, 1):
            _capi.bootstrap_accumulate_device(ctx, torch.from_numpy(m).cuda(), t, mean, m2)
        std = _capi.bootstrap_std_device(ctx, m2, count)
        ctx.sync()
        exp_mean, exp_std = B.welford(maps)
        assert _same(mean.cpu().numpy(), exp_mean), (n, k)
        assert _same(std.cpu().numpy(), exp_std), (n, k)
        assert np.isnan(exp_std).sum() == 1 and np.isnan(exp_mean).sum() == 1
        # ... and they are what numpy's own mean / std give, to rounding
        ok = ~np.isnan(exp_mean)
        assert np.allclose(exp_mean[ok], np.mean(maps, axis=0)[ok], rtol=1e-12, atol=0)
        # in place: std written over M2
        assert _capi.bootstrap_std_device(ctx, m2, count, into=m2) is m2
        ctx.sync()
        assert _same(m2.cpu().numpy(), exp_std)


def test_bad_arguments_are_refused_by_message():
    import torch
    from amico_amd import _capi, get_context
    ctx = get_context()
    L, p = _capi.lib(), _capi._dptr
    n, nS = 8, 6
    y = torch.zeros((n, nS), dtype=torch.float32, device='cuda')
    y64 = torch.zeros((n, nS), dtype=torch.float64, device='cuda')
    ye = torch.zeros((n, nS), dtype=torch.float64, device='cuda')
    yb = torch.full((n, nS), -7.0, dtype=torch.float32, device='cuda')
    m = torch.full((3, n * nS), -7.0, dtype=torch.float64, device='cuda')

    def refused(rc, text):
        msg = L.amx_last_error(ctx._h).decode()
        assert rc == _capi.AMX_E_BADARG and text in msg, (rc, msg)
    f32 = L.amx_bootstrap_resample_device_f32
    assert f32(None, p(y), p(ye), n, nS, 0, 0, 0, p(yb), None) == _capi.AMX_E_BADARG
    refused(f32(ctx._h, None, p(ye), n, nS, 0, 0, 0, p(yb), None), 'amx_bootstrap_resample: null buffer')
    refused(f32(ctx._h, p(y), p(ye), n, nS, 0, 0, 0, None, None), 'amx_bootstrap_resample: null buffer')
    refused(f32(ctx._h, p(y), p(ye), -1, nS, 0, 0, 0, p(yb), None), 'amx_bootstrap_resample: bad n_vox')
    refused(f32(ctx._h, p(y), p(ye), n, 0, 0, 0, 0, p(yb), None), 'amx_bootstrap_resample: bad nS')
    refused(f32(ctx._h, p(y), p(ye), n, nS, -1, 0, 0, p(yb), None), 'must not be negative')
    refused(f32(ctx._h, p(y), p(ye), n, nS, 0, 0, -1, p(yb), None), 'must not be negative')
    refused(f32(ctx._h, p(y), p(ye), n, nS, 0, 0, 0, p(y), None), 'must not overlap')
    refused(f32(ctx._h, p(y), p(ye), n, nS, 0, 0, 0, c_off(y, 4 * nS), None), 'must not overlap')
    refused(L.amx_bootstrap_resample_device(ctx._h, p(y64), p(ye), n, nS, 0, 0, 0, p(ye), None), 'must not overlap')
    assert f32(ctx._h, None, None, 0, nS, 0, 0, 0, None, None) == _capi.AMX_OK           # n_vox == 0: a no-op
    acc, std = L.amx_bootstrap_accumulate_device, L.amx_bootstrap_std_device
    refused(acc(ctx._h, p(m[0]), n * nS, 0, p(m[1]), p(m[2]), None), 't counts the replicates from 1')
    refused(acc(ctx._h, p(m[0]), n * nS, 1, None, p(m[2]), None), 'amx_bootstrap_accumulate: null buffer')
    refused(acc(ctx._h, p(m[0]), n * nS, 1, p(m[1]), p(m[1]), None), 'must not overlap')
    refused(acc(ctx._h, p(m[0]), -1, 1, p(m[1]), p(m[2]), None), 'amx_bootstrap_accumulate: bad n_elems')
    assert acc(ctx._h, None, 0, 1, None, None, None) == _capi.AMX_OK
    refused(std(ctx._h, p(m[1]), n * nS, 1, p(m[2]), None), 'at least 2 replicates')
    refused(std(ctx._h, None, n * nS, 2, p(m[2]), None), 'amx_bootstrap_std: null buffer')
    assert std(ctx._h, None, 0, 2, None, None) == _capi.AMX_OK
    ctx.sync()
    assert (yb.cpu().numpy() == -7.0).all() and (m.cpu().numpy() == -7.0).all() and not y.cpu().numpy().any()      # a refused call enqueues nothing
    with pytest.raises(ValueError, match='y_est must be'):
        _capi.bootstrap_resample_device(ctx, y, ye[:, :-1].contiguous(), 0, 0)
    with pytest.raises(ValueError, match='into must be'):
        _capi.bootstrap_resample_device(ctx, y, ye, 0, 0, into=y64)
    with pytest.raises(ValueError, match='mean must be'):
        _capi.bootstrap_accumulate_device(ctx, m[0], 1, m[1].cpu(), m[2])


def c_off(t, elements):
    """device pointer `elements` into tensor t"""
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + elements * t.element_size())


# ------------------------------------------------------------------ 3. the driver is the composition of its public parts
@functools.lru_cache(maxsize=None)
def _czb_fixture():
    from conftest import expand_lut, load_npz
    f = load_npz('czb_fixture.npz')
    K = {'model': 'CylinderZeppelinBall', 'wmr': expand_lut(f['wmr_slices'], f['lut_ids']), 'wmh': expand_lut(f['wmh_slices'], f['lut_ids']),
         'iso': f['iso']}
    return f, K


def _czb_directions(n, seed):
    """random directions in the LUT cells the fixture has dictionaries for"""
    from amico_amd import synthetic as S
    rng = np.random.default_rng(seed)
    ids, ht, got = _czb_fixture()[0]['lut_ids'], _htable()['htable'], []
    while sum(len(d) for d in got) < n:
        d = S.random_unit_vectors(100000, rng)
        got.append(d[np.isin(S.lut_indices(d, ht), ids)])
    return np.ascontiguousarray(np.concatenate(got)[:n])


@functools.lru_cache(maxsize=None)
def _model(model):
    """(scheme, KERNELS, upload(ctx) -> Lut, lambdas, extras): noddi 9 b0 + 90 DWI and 145 atoms; freewater the 5 + 60 volumes whose
    float32 fit takes k_freewater_fused; CylinderZeppelinBall on its fixture's orientations"""
    from amico_amd import _capi, synthetic as S
    h = _htable()
    ht = h['htable']
    if model == 'noddi':
        sch = S.make_scheme(9, ((700.0, 30), (2000.0, 60)), seed=0)
        K = S.noddi_kernels(sch, h['dirs'])
        return sch, K, lambda ctx: _capi.upload_noddi(ctx, K, ht, sch.dwi_idx), (0.5, 1e-3), (3,)
    if model == 'freewater':
        sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
        K = S.freewater_kernels(sch, h['dirs'])
        return sch, K, lambda ctx: _capi.upload_freewater(ctx, K, ht), (0.0, 1e-3), (0,)
    f, K = _czb_fixture()
    return None, K, lambda ctx: _capi.upload_czb(ctx, K, f['Rs'], ht), (0.0, 4.0), ()


@functools.lru_cache(maxsize=None)
def _signals(model, n, seed, snr=30.0):
    """noddi: float64 rows, freewater: float32 rows (the image dtype), czb: float64 rows -- shared, not modified"""
    from amico_amd import synthetic as S
    sch, K = _model(model)[:2]
    ht = _htable()['htable']
    if model == 'noddi':
        y, d = S.noddi_signals(n, K, ht, sch, seed=seed, snr=snr)
    elif model == 'freewater':
        y, d = S.freewater_signals(n, K, ht, sch, seed=seed, snr=snr)
        y = y.astype(np.float32)
    else:
        rng = np.random.default_rng(seed)
        d = _czb_directions(n, seed)
        lut = S.lut_indices(d, ht)
        w = rng.dirichlet([2.0, 2.0, 1.0], n)
        y0 = w[:, :1] * K['wmr'][rng.integers(K['wmr'].shape[0], size=n), lut].astype(np.float64) + \
            w[:, 1:2] * K['wmh'][rng.integers(K['wmh'].shape[0], size=n), lut].astype(np.float64) + w[:, 2:] * K['iso'][0].astype(np.float64)
        y = np.abs(y0 + rng.normal(scale=1 / snr, size=y0.shape) + 1j * rng.normal(scale=1 / snr, size=y0.shape))
    y.setflags(write=False)
    d.setflags(write=False)
    return y, d


def _base_fit(model, ctx, lut, yt, dt):
    """the fit with the coefficient hand-over: (maps, x, y_est), device tensors"""
    from amico_amd import _capi
    lambdas, extras = _model(model)[3:]
    out = getattr(_capi, model + '_fit_device')(ctx, lut, yt, dt, *lambdas, *extras, return_x=True)
    ye = _capi.predict_device(ctx, lut, out[-1], dt)
    ctx.sync()
    return out[0], out[-1], ye


def _replicate_maps(model, ctx, lut, y, ye, dt, samples, seed, first=0, fit=None):
    """maps of the replicates made in numpy from the downloaded y / y_est and fitted one by one: by the plain device fit, or by `fit`"""
    import torch
    from amico_amd import _capi
    lambdas, extras = _model(model)[3:]
    maps = []
    for b in range(samples):
        yb = B.resample(y, ye, seed, b, first)
        if fit is not None:
            maps.append(fit(yb))
            continue
        est = getattr(_capi, model + '_fit_device')(ctx, lut, torch.from_numpy(yb).cuda(), dt, *lambdas, *extras)[0]
        ctx.sync()
        maps.append(est.cpu().numpy())
    return maps


DRIVER = {
    'noddi wavefront kernels': ('noddi', 3000, 4, 'k_noddi', 'k_nnls_seed'),
    'noddi seeded chain': ('noddi', 24000, 3, 'k_nnls_seed<1', None),          # (the threshold is 22 528 voxels)
    'freewater fast': ('freewater', 3000, 4, 'k_freewater_fused', None),
    'czb fast': ('czb', 3000, 4, 'k_czb_lane', None),
}


@pytest.mark.parametrize('name', list(DRIVER))
def test_driver_is_the_composition_of_its_parts(name):
    import torch
    from amico_amd import _capi, bootstrap, get_context
    model, n, samples, must, must_not = DRIVER[name]
    lambdas, extras = _model(model)[3:]
    y, d = _signals(model, n, 4 if model == 'noddi' else 11 if model == 'freewater' else 3)
    ctx = get_context()
    lut = _model(model)[2](ctx)
    yt, dt = torch.from_numpy(y.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
    base, x, ye = _base_fit(model, ctx, lut, yt, dt)
    seed, first = 2 ** 63 + 5, 12345
    mean, std = bootstrap.wild_bootstrap(ctx, _capi.FIT[model], lut, yt, dt, *lambdas, extras, x, samples, seed=seed, first_voxel=first)
    ctx.sync()
    path = ctx.last_path()
    assert must in path and (must_not is None or must_not not in path), path       # the replicates take the kernels of the plain fit
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    maps = _replicate_maps(model, ctx, lut, y, ye.cpu().numpy(), dt, samples, seed, first)
    assert ctx.last_path() == path
    exp_mean, exp_std = B.welford(maps)
    assert mean.dtype == np.float64 and mean.shape == base.shape and std.shape == base.shape
    assert np.array_equal(mean, exp_mean), (name, int((mean != exp_mean).sum()))
    assert np.array_equal(std, exp_std), (name, int((std != exp_std).sum()))
    assert np.isfinite(std).all() and (std >= 0).all() and np.median(std.max(axis=1)) > 1e-4          # the replicates differ
    # neither the signals nor the base fit's tensors were touched
    assert np.array_equal(yt.cpu().numpy(), y)
    if n <= 3000:
        again = bootstrap.wild_bootstrap(ctx, _capi.FIT[model], lut, yt, dt, *lambdas, extras, x, samples, seed=seed, first_voxel=first)
        other = bootstrap.wild_bootstrap(ctx, _capi.FIT[model], lut, yt, dt, *lambdas, extras, x, samples, seed=seed + 1, first_voxel=first)
        ctx.sync()
        assert np.array_equal(again[0].cpu().numpy(), mean) and np.array_equal(again[1].cpu().numpy(), std)
        assert not np.array_equal(other[0].cpu().numpy(), mean) and not np.array_equal(other[1].cpu().numpy(), std)
    lut.close()


# ------------------------------------------------------------------ 4. one leg against the CPU oracle
@pytest.mark.parametrize('model', ['noddi', 'freewater'])
def test_bootstrap_against_the_oracle(model):
    """The replicates are made in numpy from the DEVICE's prediction and fitted by the oracle; mean map: every voxel within CAP and
    SHARE of them within TOL, the bounds of a single fit (a mean of maps that each move by at most e moves by at most e).  Std map:
    the same share with both bounds scaled by 2 sqrt(B / (B - 1)): std is the norm of the centred replicate vector over sqrt(B - 1),
    centring has norm <= 1 but moves with the mean as well (factor 2), and a vector of B entries that each move by e moves by
    sqrt(B) e."""
    import torch
    from amico_amd import _capi, bootstrap, get_context
    from oracle import oracle
    n, samples, seed = 1037, 4, 0
    sch, K, upload, lambdas, extras = _model(model)
    ht = _htable()['htable']
    y, d = _signals(model, n, 21)
    ctx = get_context()
    lut = upload(ctx)
    yt, dt = torch.from_numpy(y.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
    base, x, ye = _base_fit(model, ctx, lut, yt, dt)
    mean, std = bootstrap.wild_bootstrap(ctx, _capi.FIT[model], lut, yt, dt, *lambdas, extras, x, samples, seed=seed)
    ctx.sync()
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    nt = min(16, os.cpu_count() or 1)
    if model == 'noddi':
        fit = lambda yb: oracle.noddi_fit(yb.astype(np.float64), d, K, ht, sch.dwi_idx, *lambdas, nthreads=nt)['estimates']      # noqa: E731
    else:
        fit = lambda yb: oracle.freewater_fit(yb.astype(np.float64), d, K, ht, *lambdas, nthreads=nt)['estimates']             # noqa: E731
    ref_mean, ref_std = B.welford(_replicate_maps(model, ctx, lut, y, ye.cpu().numpy(), dt, samples, seed, fit=fit))
    scale = 2.0 * np.sqrt(samples / (samples - 1.0))
    dm, ds = np.abs(mean - ref_mean).max(axis=1), np.abs(std - ref_std).max(axis=1)
    print(f'{model}: mean map max {dm.max():.3e}, within {TOL:g}: {100 * (dm < TOL).mean():.2f}%; std map max {ds.max():.3e}, within '
          f'{scale * TOL:.2g}: {100 * (ds < scale * TOL).mean():.2f}%; median std {np.median(std, axis=0)}')
    assert dm.max() < CAP and (dm < TOL).mean() >= SHARE
    assert ds.max() < scale * CAP and (ds < scale * TOL).mean() >= SHARE
    lut.close()


# ------------------------------------------------------------------ 5. sanity of the statistic
def test_noisier_signals_have_the_larger_standard_error():
    """Free-Water, 1 037 voxels, B = 20: the median std of the FW map at SNR 10 exceeds the median at SNR 50 (the noise is five times
    as large; the CPU oracle run on the same replicates gives medians of 0.078 and 0.019)"""
    import torch
    from amico_amd import _capi, bootstrap, get_context
    sch, K, upload, lambdas, extras = _model('freewater')
    ctx = get_context()
    lut = upload(ctx)
    med = {}
    for snr in (10.0, 50.0):
        y, d = _signals('freewater', 1037, 11, snr)
        yt, dt = torch.from_numpy(y.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
        base, x, ye = _base_fit('freewater', ctx, lut, yt, dt)
        mean, std = bootstrap.wild_bootstrap(ctx, _capi.FIT['freewater'], lut, yt, dt, *lambdas, extras, x, 20)
        ctx.sync()
        med[snr] = float(np.median(std.cpu().numpy()[:, 1]))
    print(f'median std of FW: SNR 10 {med[10.0]:.4f}, SNR 50 {med[50.0]:.4f}, ratio {med[10.0] / med[50.0]:.2f}')
    assert med[10.0] > med[50.0] > 0
    lut.close()


# ------------------------------------------------------------------ 6. Evaluation
def _image(model, shape):
    from amico_amd import synthetic as S
    sch, K = _model(model)[:2]
    ht = _htable()['htable']
    n = int(np.prod(shape))
    y, d = (S.noddi_signals if model == 'noddi' else S.freewater_signals)(n, K, ht, sch, seed=2)
    rng = np.random.default_rng(3)
    mask = (rng.uniform(size=shape) < 0.7).astype(np.uint8)
    mask[:, :, 0] = 0
    return sch, K, ht, (y.reshape(shape + (-1,)) * 640.0).astype(np.float32), mask, d.reshape(shape + (3,))


@pytest.mark.parametrize('model', ['noddi', 'freewater'])
def test_evaluation_bootstrap(model):
    import amico_amd
    from amico_amd import _capi, bootstrap, get_context
    shape = (12, 11, 10)
    sch, K, ht, img, mask, dirs = _image(model, shape)
    sel = mask == 1
    n = int(sel.sum())
    n_maps = 3 if model == 'noddi' else 2
    ticks = []

    def run(**cfg):
        ae = amico_amd.Evaluation()
        for key, v in cfg.items():
            ae.set_config(key, v)
        ae.set_data(img, sch, mask, dirs)
        ae.set_model('NODDI' if model == 'noddi' else 'FreeWater')
        ae.set_kernels(K, ht)
        return ae, ae.fit()
    ae, res = run(bootstrap_samples=4, bootstrap_seed=7, progress_callback=lambda done, total: ticks.append((done, total)))
    for key in ('MAPs_std', 'MAPs_boot_mean'):
        vol = ae.RESULTS[key]
        assert vol.dtype == np.float32 and vol.shape == shape + (n_maps,) and not vol[~sel].any() and np.isfinite(vol).all()
    for key in ('estimates_std', 'estimates_boot_mean'):
        assert res[key].dtype == np.float64 and res[key].shape == (n, n_maps)
    assert ae._y is None                                    # the signals never came to the host
    assert np.array_equal(ae.RESULTS['MAPs_std'][sel], res['estimates_std'].astype(np.float32))
    assert np.array_equal(ae.RESULTS['MAPs_boot_mean'][sel], res['estimates_boot_mean'].astype(np.float32))
    assert ae.RESULTS['MAPs_std'][sel].max() > 1e-4 and len(ticks) > 1
    # the bootstrap run by hand on the tensors the fit read
    ctx = get_context()
    lut = _model(model)[2](ctx)
    lambdas, extras = _model(model)[3:]
    yt, dt = ae._dev['y'], ae._dev['dirs']
    assert yt.dtype.is_floating_point and yt.shape[0] == n
    base, x, ye = _base_fit(model, ctx, lut, yt, dt)
    mean, std = bootstrap.wild_bootstrap(ctx, _capi.FIT[model], lut, yt, dt, *lambdas, extras, x, 4, seed=7)
    ctx.sync()
    assert np.array_equal(res['estimates_std'], std.cpu().numpy()) and np.array_equal(res['estimates_boot_mean'], mean.cpu().numpy())
    assert np.array_equal(ae.RESULTS['MAPs_std'], ae._prep.scatter(std.cpu().numpy()))
    assert np.array_equal(ae.RESULTS['MAPs_boot_mean'], ae._prep.scatter(mean.cpu().numpy()))
    assert np.array_equal(res['estimates'], base.cpu().numpy())
    # without the key: neither entry, the same maps bit for bit
    ae0, res0 = run()
    assert not {'MAPs_std', 'MAPs_boot_mean'} & set(ae0.RESULTS) and not {'estimates_std', 'estimates_boot_mean'} & set(res0)
    assert type(res0) is dict or model == 'freewater'
    assert np.array_equal(ae0.RESULTS['MAPs'], ae.RESULTS['MAPs']) and np.array_equal(res0['estimates'], res['estimates'])
    # beside the predicted signal: one fit hands the coefficients to both
    ae2, res2 = run(bootstrap_samples=4, bootstrap_seed=7, doSavePredictedSignal=True)
    assert list(res2)[-1] == 'y_est' and 'DWI_predicted' in ae2.RESULTS
    assert np.array_equal(ae2.RESULTS['MAPs_std'], ae.RESULTS['MAPs_std']) and np.array_equal(ae2.RESULTS['MAPs'], ae.RESULTS['MAPs'])
    assert np.array_equal(res2['y_est'], ye.cpu().numpy())
    lut.close()


def test_evaluation_refusals():
    import amico_amd
    shape = (4, 4, 3)
    sch, K, ht, img, mask, dirs = _image('freewater', shape)

    def make(samples):
        ae = amico_amd.Evaluation()
        ae.set_config('bootstrap_samples', samples)
        ae.set_data(img, sch, np.ones(shape, np.uint8), dirs)
        ae.set_model('FreeWater')
        ae.set_kernels(K, ht)
        return ae
    amico_amd.set_devices([0, 0])                          # a device named twice: two contexts
    try:
        ae = make(4)
        with pytest.raises(NotImplementedError, match='several devices'):
            ae.fit()
        assert ae._dev is None and ae.RESULTS is None      # nothing was uploaded
    finally:
        amico_amd.set_devices(None)
    ae = make(1)
    with pytest.raises(ValueError, match='bootstrap_samples'):
        ae.fit()
    assert ae._dev is None and ae.RESULTS is None
    # an assigned y: the model's fit has no device-resident signals to resample
    ae = make(4)
    ae.fit()
    ae.y = ae.y.copy()
    with pytest.raises(NotImplementedError, match='assigned evaluation.y'):
        ae.model.fit(ae)
