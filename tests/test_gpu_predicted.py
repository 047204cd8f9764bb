"""The predicted signal y_est = A x on the GPU (include/amico_amd.h: amx_predict_device / amx_prep_predicted_device): the kernel alone,
bit for bit against the numpy restatement of tests/predicted_np.py; through each model's default fast fit against the CPU oracle;
Evaluation's 'doSavePredictedSignal'; the refusals.  Every voxel is compared.
TOL is the bound tests/test_gpu_fw_corrected.py holds y_corrected to: the prediction is linear in x with 0 <= A <= 1, and the RMSE is
1-Lipschitz in y_est, so both bounds of part 2 follow from the coefficients' own agreement with the oracle."""
import functools
import os

import numpy as np
import pytest

import predicted_np as P

pytestmark = pytest.mark.gpu

TOL = 1e-6
COUNTS = (1, 63, 65, 1037)          # one voxel, a block less one, a block and one, 16 blocks and a remainder
CAP = 16                            # non-zeros per voxel the kernel keeps on chip (kPredCap): 16 fit, 17 do not


@functools.lru_cache(maxsize=None)
def _htable():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'htable500.npz'), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def _czb_fixture():
    from conftest import expand_lut, load_npz
    f = load_npz('czb_fixture.npz')
    K = {'model': 'CylinderZeppelinBall', 'wmr': expand_lut(f['wmr_slices'], f['lut_ids']), 'wmh': expand_lut(f['wmh_slices'], f['lut_ids']),
         'iso': f['iso']}
    return f, K


@functools.lru_cache(maxsize=None)
def _dictionary(model):
    """(scheme, KERNELS, upload(ctx) -> Lut, fit extras): small dictionaries of amico_amd.synthetic on the 500 directions of htable500;
    CylinderZeppelinBall as tests/test_gpu_czb.py builds it (the fixture's orientations)"""
    from amico_amd import _capi, synthetic as S
    h = _htable()
    ht = h['htable']
    if model == 'noddi':                                   # 9 b0 + 90 DWI, 145 atoms
        sch = S.make_scheme(9, ((700.0, 30), (2000.0, 60)), seed=0)
        K = S.noddi_kernels(sch, h['dirs'])
        return sch, K, lambda ctx: _capi.upload_noddi(ctx, K, ht, sch.dwi_idx), None
    if model == 'freewater':                               # 1 + 64, 11 atoms
        sch = S.make_scheme(1, ((1000.0, 64),), seed=3)
        K = S.freewater_kernels(sch, h['dirs'])
        return sch, K, lambda ctx: _capi.upload_freewater(ctx, K, ht), None
    if model == 'sandi':                                   # 6 rows, 15 atoms
        sch = S.directional_average_scheme(S.make_sandi_scheme(ndir_per_shell=24, n_b0=4))
        K, Rs, d_in, d_isos = S.sandi_kernels(sch)
        return sch, K, lambda ctx: _capi.upload_sandi(ctx, K, Rs, d_in, d_isos), (Rs, d_in, d_isos)
    f, K = _czb_fixture()
    return None, K, lambda ctx: _capi.upload_czb(ctx, K, f['Rs'], ht), f['Rs']


def _directions(model, n, seed):
    """random directions (CylinderZeppelinBall: in the LUT cells its fixture has dictionaries for); None for SANDI"""
    from amico_amd import synthetic as S
    if model == 'sandi':
        return None
    rng = np.random.default_rng(seed)
    if model != 'czb':
        return S.random_unit_vectors(n, rng)
    ids, ht, got = _czb_fixture()[0]['lut_ids'], _htable()['htable'], []
    while sum(len(d) for d in got) < n:
        d = S.random_unit_vectors(100000, rng)
        got.append(d[np.isin(S.lut_indices(d, ht), ids)])
    return np.ascontiguousarray(np.concatenate(got)[:n])


def _coefficients(n, n_atoms, seed):
    """hand-made rows, cycling: a few non-zeros, none, one, exactly CAP, CAP + 1, every atom (beyond any capacity), a NaN among a few"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, n_atoms))
    for i in range(n):
        kind = i % 7
        k = {0: 4, 1: 0, 2: 1, 3: CAP, 4: CAP + 1, 5: n_atoms, 6: 3}[kind]
        at = rng.choice(n_atoms, size=min(k, n_atoms), replace=False)
        x[i, at] = rng.uniform(0.01, 1.0, len(at))
        if kind == 6:
            x[i, rng.integers(n_atoms)] = np.nan
    x[-1, :] = 0.0
    x[-1, n_atoms - 1] = 0.75                              # the last atom alone, in the last voxel
    return x


@functools.lru_cache(maxsize=None)
def _kernel_case(model):
    """directions, coefficients and the restatement's rows for the largest count: computed once, shared, never modified"""
    sch, K, upload, _ = _dictionary(model)
    n = COUNTS[-1]
    n_atoms = len(P.columns(K))
    d = _directions(model, n, seed=5)
    x = _coefficients(n, n_atoms, seed=7)
    idx = None if d is None else P.lut_index(d, _htable()['htable'], 500)
    ref = P.predict_rows(K, x, idx)
    for a in (x, ref) + (() if d is None else (d,)):
        a.setflags(write=False)
    assert idx is None or (idx >= 0).all()
    assert np.isnan(ref[6]).all() and not ref[1].any() and np.isfinite(ref[0]).all() and ref[0].any()
    return d, x, ref


# ------------------------------------------------------------------ 1. the kernel alone, bit for bit
@pytest.mark.parametrize('model', ['noddi', 'freewater', 'sandi', 'czb'])
def test_predict_kernel_equals_the_restatement(model):
    import torch
    from amico_amd import _capi, get_context
    sch, K, upload, _ = _dictionary(model)
    d, x, ref = _kernel_case(model)
    ctx = get_context()
    lut = upload(ctx)
    assert lut.nS == ref.shape[1] and lut.n_atoms == x.shape[1]
    for n in COUNTS:
        # (the first n voxels of the case: a voxel's row depends on nothing but its own coefficients and direction)
        xt = torch.from_numpy(x[:n].copy()).cuda()
        dt = None if d is None else torch.from_numpy(d[:n].copy()).cuda()
        got = _capi.predict_device(ctx, lut, xt, dt)
        ctx.sync()
        got = got.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (n, lut.nS)
        bad = int((~((got == ref[:n]) | (np.isnan(got) & np.isnan(ref[:n])))).sum())
        assert np.array_equal(got, ref[:n], equal_nan=True), (model, n, bad)
        if model == 'noddi':
            # the AMX_F_DEBUG_X layout: x_stride = 3 n_atoms, x_offset = 2 n_atoms; rows 0 and 1 hold other stages' coefficients
            x3 = np.random.default_rng(n).uniform(0.0, 1.0, (n, 3, x.shape[1]))
            x3[:, 2, :] = x[:n]
            got3 = _capi.predict_device(ctx, lut, torch.from_numpy(x3).cuda(), dt)
            ctx.sync()
            assert np.array_equal(got3.cpu().numpy(), ref[:n], equal_nan=True), (model, n, 'strided')
    lut.close()


def test_voxel_skipped_for_its_direction_gets_a_row_of_zeros():
    import torch
    from amico_amd import _capi, get_context
    sch, K, upload, _ = _dictionary('freewater')
    d, x, ref = _kernel_case('freewater')
    ctx = get_context()
    lut = upload(ctx)
    db = d[:70].copy()
    db[5] = np.nan
    got = _capi.predict_device(ctx, lut, torch.from_numpy(x[:70].copy()).cuda(), torch.from_numpy(db).cuda())
    with pytest.raises(RuntimeError, match='index out of bounds'):
        ctx.sync()
    got = got.cpu().numpy()
    exp = ref[:70].copy()
    exp[5] = 0.0
    assert np.array_equal(got, exp, equal_nan=True) and not got[5].any()
    lut.close()


@pytest.mark.parametrize('order', ['C', 'F'])
@pytest.mark.parametrize('model', ['noddi', 'freewater', 'sandi'])
def test_predicted_volume_kernel(model, order):
    """12 x 10 x 8 image with holes in the mask: float32(m * rows) scattered, exactly 0 elsewhere, on a buffer pre-filled with a sentinel"""
    import torch
    from amico_amd import _capi, get_context, prep
    sch, K, upload, _ = _dictionary(model)
    d_all, x_all, ref_all = _kernel_case(model)
    shape = (12, 10, 8)
    rng = np.random.default_rng(3)
    mask = (rng.uniform(size=shape) < 0.7).astype(np.uint8)
    mask[:, :, 0] = 0                                       # a slab without a masked voxel
    mask[2, 1, 1], mask[3, 1, 1], mask[4, 2, 1] = 1, 2, 1   # a 2 counts as unmasked
    sel = mask == 1
    n = int(sel.sum())
    assert 64 < n < len(x_all)
    ctx = get_context()
    lut = upload(ctx)
    n_out = lut.nS
    sp = prep.SignalPreparation(sch, np.zeros(shape + (n_out,), dtype=np.float32, order=order), mask, do_normalize=False, ctx=ctx)
    plan = sp._plan
    assert sp.n_vox == n and sp.n_out == n_out
    x, rows = x_all[:n], ref_all[:n]
    xt = torch.from_numpy(x.copy()).cuda()
    dt = None if d_all is None else torch.from_numpy(d_all[:n].copy()).cuda()
    mb0 = rng.uniform(300.0, 900.0, n).astype(np.float32)
    mt = torch.from_numpy(mb0).cuda()
    for rescale in (False, True):
        m64 = mb0.astype(np.float64) if rescale else np.ones(n)
        exp = np.zeros(shape + (n_out,), dtype=np.float32)
        exp[sel] = (m64[:, None] * rows).astype(np.float32)
        vol = torch.full(shape + (n_out,), -7.0, dtype=torch.float32, device='cuda')
        plan.predicted_device(lut, xt, vol, dt, mt if rescale else None)
        ctx.sync()
        got = vol.cpu().numpy()
        assert np.array_equal(got, exp, equal_nan=True), (model, order, rescale, int((got != exp).sum()))
        assert not got[~sel].any() and np.isnan(got[sel][6]).all() and got[sel][0].any()
    lut.close()


# ------------------------------------------------------------------ 2. through the default fast fit, against the oracle
def _czb_signals(n, seed):
    f, K = _czb_fixture()
    ht = _htable()['htable']
    from amico_amd import synthetic as S
    rng = np.random.default_rng(seed)
    d = _directions('czb', n, seed)
    lut = S.lut_indices(d, ht)
    w = rng.dirichlet([2.0, 2.0, 1.0], n)
    y0 = w[:, :1] * K['wmr'][rng.integers(K['wmr'].shape[0], size=n), lut].astype(np.float64) + \
        w[:, 1:2] * K['wmh'][rng.integers(K['wmh'].shape[0], size=n), lut].astype(np.float64) + w[:, 2:] * K['iso'][0].astype(np.float64)
    return np.abs(y0 + rng.normal(scale=1 / 20.0, size=y0.shape) + 1j * rng.normal(scale=1 / 20.0, size=y0.shape)), d


# name: (model, voxels, rmse asked of the device, lambdas, what ctx.last_path() must name (None: whatever it takes), what it must not)
# Every fit runs with return_x and rmse=True and keeps its default fast path -- the NODDI chain and k_sandi_rows are not gated on the
# flag.  Free-Water's and CylinderZeppelinBall's fast kernels are the maps-only ones (small_route, csrc/amx_small_route.hpp: the refill
# and the fast route exclude AMX_F_RMSE): for them the fast path is run without the error map, and a second case runs WITH it on whatever
# kernels that takes -- doComputeRMSE beside doSavePredictedSignal is what a user looking at residuals sets --, same bounds.
FITS = {
    'noddi seeded chain': ('noddi', 24000, True, (0.5, 1e-3), 'k_nnls_seed<1', None),         # (the threshold is 22 528 voxels)
    'noddi wavefront kernels': ('noddi', 3000, True, (0.5, 1e-3), 'k_noddi', 'k_nnls_seed'),
    'freewater fast': ('freewater', 3000, False, (0.0, 1e-3), 'k_freewater_fused', None),
    'freewater rmse': ('freewater', 3000, True, (0.0, 1e-3), None, 'k_freewater_fused'),
    'sandi': ('sandi', 3000, True, (0.0, 5e-3), 'k_sandi_rows', None),
    'czb fast': ('czb', 3000, False, (0.0, 4.0), 'k_czb_lane', None),
    'czb rmse': ('czb', 3000, True, (0.0, 4.0), None, 'k_czb_lane'),
}


@functools.lru_cache(maxsize=None)
def _fit_signals(model):
    """signals, directions and the oracle's coefficients, prediction and RMSE: once per model on its largest call, shared, not modified.
    Free-Water's scheme here is the 5 + 60 volumes whose float32 fit takes k_freewater_fused (the kernel test's 1 + 64 is another path)."""
    from amico_amd import _capi, synthetic as S
    from oracle import oracle
    h = _htable()
    ht = h['htable']
    nt = min(16, os.cpu_count() or 1)
    n = max(v[1] for v in FITS.values() if v[0] == model)
    if model == 'noddi':
        sch, K, upload, _ = _dictionary(model)
        y, d = S.noddi_signals(n, K, ht, sch, seed=4)
        ref = oracle.noddi_fit(y, d, K, ht, sch.dwi_idx, 0.5, 1e-3, rmse=True, nthreads=nt, return_x=True)
        x = ref['x'][:, 2, :]
    elif model == 'freewater':
        sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
        K = S.freewater_kernels(sch, h['dirs'])
        upload = lambda ctx: _capi.upload_freewater(ctx, K, ht)       # noqa: E731
        y, d = S.freewater_signals(n, K, ht, sch, seed=11)
        y = y.astype(np.float32)
        ref = oracle.freewater_fit(y.astype(np.float64), d, K, ht, 0.0, 1e-3, rmse=True, nthreads=nt, return_x=True)
        x = ref['x']
    elif model == 'sandi':
        sch, K, upload, (Rs, d_in, d_isos) = _dictionary(model)
        y, d = S.sandi_signals(n, K, sch, seed=3), None
        ref = oracle.sandi_fit(y, K, Rs, d_in, d_isos, 0.0, 5e-3, rmse=True, nthreads=nt, return_x=True)
        x = ref['x']
    else:
        sch, K, upload, Rs = _dictionary(model)
        y, d = _czb_signals(n, seed=3)
        ref = oracle.czb_fit(y, d, K, Rs, ht, 0.0, 4.0, rmse=True, nthreads=nt, return_x=True)
        x = ref['x']
    assert ref['err'] == 0
    idx = None if d is None else P.lut_index(d, ht, 500)
    yest = P.predict_rows(K, x, idx)                       # A[idx] @ x of the oracle's coefficients
    y64 = y.astype(np.float64)
    # the oracle's RMSE is the residual of this very prediction (its own summation order: to rounding)
    assert np.abs(np.sqrt(np.mean((y64 - yest) ** 2, axis=1)) - ref['rmse']).max() < 1e-12
    for a in (y, yest, ref['rmse'], ref['estimates']) + (() if d is None else (d,)):
        a.setflags(write=False)
    return K, upload, y, d, yest, ref


@pytest.mark.parametrize('name', list(FITS))
def test_prediction_of_the_fast_fit_against_the_oracle(name):
    """The fit runs with the coefficient hand-over and, wherever that keeps the path under test, with rmse=True (the table above); the
    path is asserted from last_path(); then the rows form predicts from what the fit left.  Both bounds are against the oracle: the
    prediction itself, and the RMSE of its residual against the oracle's RMSE (the device's own error map, where asked, as well)."""
    import torch
    from amico_amd import _capi, get_context
    model, n, want_rmse, (lam1, lam2), must, must_not = FITS[name]
    K, upload, y, d, yest_ref, ref = _fit_signals(model)
    ctx = get_context()
    lut = upload(ctx)
    yt = torch.from_numpy(y[:n].copy()).cuda()
    dt = None if d is None else torch.from_numpy(d[:n].copy()).cuda()
    fit = getattr(_capi, model + '_fit_device')
    args = (ctx, lut, yt) + (() if dt is None else (dt,)) + (lam1, lam2) + {'noddi': (3,), 'freewater': (False,)}.get(model, ())
    out = fit(*args, rmse=want_rmse, return_x=True)
    ctx.sync()
    path = ctx.last_path()
    assert (must is None or must in path) and (must_not is None or must_not not in path), path
    est, xd = out[0].cpu().numpy(), out[-1]
    plain = fit(*args, rmse=want_rmse)
    ctx.sync()
    assert ctx.last_path() == path                         # asking for the coefficients changes no kernel ...
    assert np.array_equal(plain[0].cpu().numpy(), est, equal_nan=True)      # ... and not a bit of the maps
    got = _capi.predict_device(ctx, lut, xd, dt)
    ctx.sync()
    got = got.cpu().numpy()
    worst = np.abs(got - yest_ref[:n]).max()
    rmse = np.sqrt(np.mean((y[:n].astype(np.float64) - got) ** 2, axis=1))
    worst_r = np.abs(rmse - ref['rmse'][:n]).max()
    print(f'{name}: {n} voxels [{path}], max |y_est - oracle| {worst:.3e}, max |rmse(y_est) - oracle| {worst_r:.3e}, mean rmse {rmse.mean():.3e}')
    assert got.shape == (n, lut.nS) and np.isfinite(got).all()
    assert worst < TOL
    assert worst_r < TOL
    if want_rmse:
        # the error map the same fit wrote is the residual of this prediction too
        dev_rmse = out[1].cpu().numpy()
        assert np.array_equal(plain[1].cpu().numpy(), dev_rmse, equal_nan=True)
        worst_d = np.abs(dev_rmse - rmse).max()
        print(f'{name}: max |rmse of the fit - rmse(y_est)| {worst_d:.3e}')
        assert worst_d < TOL
    lut.close()


# ------------------------------------------------------------------ 3. Evaluation
def _count_predict_calls(monkeypatch):
    from amico_amd import _capi
    calls, real = [], _capi.predict_device

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(_capi, 'predict_device', spy)
    return calls


def _check_evaluation(ae, res, img, sel, normalize, calls, close):
    vol = ae.RESULTS['DWI_predicted']
    n_out = ae._prep.n_out
    assert vol.dtype == np.float32 and vol.shape == img.shape[:3] + (n_out,) and not vol[~sel].any()
    assert 'y_est' in res and list(res)[-1] == 'y_est' and not calls          # a key from the start, the rows not made
    assert ae._y is None                                   # the signals never came to the host
    rows = res['y_est']
    assert res['y_est'] is rows and calls == [1]           # made once, when read
    assert rows.dtype == np.float64 and rows.shape == (int(sel.sum()), n_out) and np.isfinite(rows).all()
    m = ae.mean_b0s.astype(np.float64)[:, None] if normalize else 1.0
    assert np.array_equal(vol[sel], (m * rows).astype(np.float32))
    if close:
        # it is the prediction of THIS fit: close to the signals the fit saw (SNR 30 data: residual of a few percent).  Not so for SANDI,
        # whose rescaled coefficients meet the normalised dictionary (the quirk of models.pyx:1570-1571 the error maps reproduce)
        y = ae.y
        assert np.sqrt(np.mean((y - rows) ** 2)) < 0.1 * np.sqrt(np.mean(y ** 2))


@pytest.mark.parametrize('normalize', [True, False])
def test_evaluation_noddi_predicted_signal(monkeypatch, normalize):
    import amico_amd
    from amico_amd import synthetic as S
    sch, K, _, _ = _dictionary('noddi')
    ht = _htable()['htable']
    shape = (12, 10, 7)
    mask = np.ones(shape, dtype=np.uint8)
    mask[:, :, 0] = 0
    mask[3, 4, 2] = 0
    sel = mask == 1
    y, d = S.noddi_signals(int(np.prod(shape)), K, ht, sch, seed=2)
    img = (y.reshape(shape + (-1,)) * (640.0 if normalize else 1.0)).astype(np.float32)
    calls = _count_predict_calls(monkeypatch)
    ae = amico_amd.Evaluation()
    ae.set_config('doNormalizeSignal', normalize)
    ae.set_config('doSavePredictedSignal', True)
    ae.set_data(img, sch, mask, d.reshape(shape + (3,)))
    ae.set_model('NODDI')
    ae.set_kernels(K, ht)
    res = ae.fit()
    _check_evaluation(ae, res, img, sel, normalize, calls, True)
    maps = ae.RESULTS['MAPs']
    # without the key: neither the volume nor the rows, and the same maps
    ae.set_config('doSavePredictedSignal', None)
    res0 = ae.fit()
    assert 'DWI_predicted' not in ae.RESULTS and 'y_est' not in res0 and type(res0) is dict and calls == [1]
    assert np.array_equal(ae.RESULTS['MAPs'], maps) and 'predict' not in ae._dev


def _sandi_image():
    from amico_amd import synthetic as S
    full = S.make_sandi_scheme(ndir_per_shell=24, n_b0=4)
    rng = np.random.default_rng(5)
    shape = (14, 9, 6)
    avg = S.directional_average_scheme(full)
    K = S.sandi_kernels(avg)[0]
    ya = S.sandi_signals(int(np.prod(shape)), K, avg, seed=3)
    img = np.zeros(shape + (full.nS,), dtype=np.float32)
    img[..., full.b0_idx] = 1000.0
    for k, sh in enumerate(sorted(full.shells, key=lambda s: s['b'])):
        img[..., sh['idx']] = (1000.0 * ya[:, k + 1].reshape(shape + (1,)) *
                               (1.0 + 0.05 * rng.standard_normal(shape + (len(sh['idx']),)))).astype(np.float32)
    img = np.asfortranarray(img)
    mask = (rng.uniform(size=shape) < 0.8).astype(np.uint8)
    return full, img, mask, shape


def test_evaluation_sandi_predicted_signal_with_directional_average(monkeypatch):
    import amico_amd
    from amico_amd import synthetic as S
    full, img, mask, shape = _sandi_image()
    calls = _count_predict_calls(monkeypatch)
    ae = amico_amd.Evaluation()
    ae.set_config('doDirectionalAverage', True)
    ae.set_config('doSavePredictedSignal', True)
    ae.set_data(img, full, mask)
    ae.set_model('SANDI')
    ae.set_kernels(S.sandi_kernels(ae.scheme)[0])
    res = ae.fit()
    assert ae.RESULTS['DWI_predicted'].shape == shape + (6,)
    _check_evaluation(ae, res, img, mask == 1, True, calls, False)


# ------------------------------------------------------------------ 4. refusals
def test_bad_arguments_are_refused_by_message():
    import torch
    from amico_amd import _capi, get_context, prep
    ctx = get_context()
    L, p = _capi.lib(), _capi._dptr
    sch, K, upload, _ = _dictionary('freewater')
    fw = upload(ctx)
    sa = _dictionary('sandi')[2](ctx)
    n = 8
    x = torch.zeros((n, fw.n_atoms), dtype=torch.float64, device='cuda')
    xs = torch.zeros((n, sa.n_atoms), dtype=torch.float64, device='cuda')
    d = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
    d[:, 2] = 1.0
    out = torch.full((n, fw.nS), -7.0, dtype=torch.float64, device='cuda')

    def refused(rc, text):
        msg = L.amx_last_error(ctx._h).decode()
        assert rc == _capi.AMX_E_BADARG and text in msg, (rc, msg)
    na = fw.n_atoms
    refused(L.amx_predict_device(ctx._h, fw._h, None, na, 0, p(d), n, p(out), None), 'amx_predict: null buffer')
    refused(L.amx_predict_device(ctx._h, fw._h, p(x), na, 0, p(d), n, None, None), 'amx_predict: null buffer')
    refused(L.amx_predict_device(ctx._h, None, p(x), na, 0, p(d), n, p(out), None), 'amx_predict: not a dictionary of this ctx')
    refused(L.amx_predict_device(ctx._h, fw._h, p(x), na, 0, None, n, p(out), None), 'a FreeWater dictionary needs the directions')
    refused(L.amx_predict_device(ctx._h, sa._h, p(xs), sa.n_atoms, 0, p(d), n, p(out), None), 'a SANDI dictionary takes no directions')
    refused(L.amx_predict_device(ctx._h, fw._h, p(x), na - 1, 0, p(d), n, p(out), None), 'x_stride is smaller than x_offset + n_atoms')
    refused(L.amx_predict_device(ctx._h, fw._h, p(x), 3 * na, 2 * na + 1, p(d), n, p(out), None), 'x_stride is smaller than x_offset + n_atoms')
    refused(L.amx_predict_device(ctx._h, fw._h, p(x), na, 0, p(d), -1, p(out), None), 'amx_predict: bad n_vox')
    # volume form
    shape = (2, 2, 2)
    sp = prep.SignalPreparation(sch, np.zeros(shape + (fw.nS,), dtype=np.float32), np.ones(shape, dtype=np.uint8), do_normalize=False, ctx=ctx)
    plan = sp._plan
    vol = torch.full(shape + (fw.nS,), -7.0, dtype=torch.float32, device='cuda')
    refused(L.amx_prep_predicted_device(ctx._h, None, fw._h, p(x), na, 0, p(d), None, p(vol), None), 'amx_prep_predicted: not a plan of this ctx')
    refused(L.amx_prep_predicted_device(ctx._h, plan._h, fw._h, p(x), na, 0, p(d), None, None, None), 'amx_prep_predicted: null buffer')
    refused(L.amx_prep_predicted_device(ctx._h, plan._h, fw._h, None, na, 0, p(d), None, p(vol), None), 'amx_prep_predicted: null buffer')
    refused(L.amx_prep_predicted_device(ctx._h, plan._h, fw._h, p(x), na, 0, None, None, p(vol), None), 'a FreeWater dictionary needs the directions')
    refused(L.amx_prep_predicted_device(ctx._h, plan._h, fw._h, p(x), na - 1, 0, p(d), None, p(vol), None), 'x_stride is smaller than x_offset + n_atoms')
    refused(L.amx_prep_predicted_device(ctx._h, plan._h, sa._h, p(xs), sa.n_atoms, 0, None, None, p(vol), None), 'another number of volumes')
    ctx.sync()
    assert (out.cpu().numpy() == -7.0).all() and (vol.cpu().numpy() == -7.0).all()      # a refused call enqueues nothing
    with pytest.raises(ValueError, match='x must be a contiguous float64 device tensor'):
        _capi.predict_device(ctx, fw, x[:, :-1].contiguous(), d)
    # tensors on another device than x (here: the host) never reach the kernel
    with pytest.raises(ValueError, match='DIRs must be'):
        _capi.predict_device(ctx, fw, x, d.cpu())
    with pytest.raises(ValueError, match='volume must be'):
        plan.predicted_device(fw, x, vol.cpu(), d)
    with pytest.raises(ValueError, match='mean_b0 must be'):
        plan.predicted_device(fw, x, vol, d, torch.ones(n, dtype=torch.float32))
    fw.close()
    sa.close()


def test_model_that_leaves_no_coefficients_is_not_implemented():
    """a plug-in whose fit() does not go through BaseModel._run: one sentence, not a KeyError"""
    import amico_amd
    from amico_amd import synthetic as S
    full, img, mask, shape = _sandi_image()

    class PlugIn(amico_amd.SANDI):
        def fit(self, evaluation):
            return {'estimates': np.zeros((evaluation._dev['y'].shape[0], 6))}
    ae = amico_amd.Evaluation()
    ae.set_config('doDirectionalAverage', True)
    ae.set_config('doSavePredictedSignal', True)
    ae.set_data(img, full, mask)
    ae.set_model('SANDI')
    ae.model = PlugIn()
    ae.set_kernels(S.sandi_kernels(ae.scheme)[0])
    with pytest.raises(NotImplementedError, match='left no coefficients'):
        ae.fit()


def test_assigned_y_with_the_key_is_not_implemented():
    import amico_amd
    ae = amico_amd.Evaluation()
    ae.set_config('doSavePredictedSignal', True)
    ae.y = np.zeros((4, 6))
    ae.nthreads = 1
    model = amico_amd.SANDI()
    with pytest.raises(NotImplementedError, match='doSavePredictedSignal'):
        model.fit(ae)


def test_evaluation_freewater_corrected_and_predicted_together(monkeypatch):
    """doSaveCorrectedDWI, doSavePredictedSignal and doComputeRMSE in one fit: x and x_iso both come back from it, both volumes are
    made in HBM, both rows are lazy and made one by one"""
    import amico_amd
    from amico_amd import synthetic as S
    h = _htable()
    ht = h['htable']
    sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
    K = S.freewater_kernels(sch, h['dirs'])
    shape = (12, 10, 7)
    mask = np.ones(shape, dtype=np.uint8)
    mask[:, :, 0] = 0
    sel = mask == 1
    y, d = S.freewater_signals(int(np.prod(shape)), K, ht, sch, seed=2)
    img = (y.reshape(shape + (-1,)) * 640.0).astype(np.float32)
    calls = _count_predict_calls(monkeypatch)

    def run(**cfg):
        ae = amico_amd.Evaluation()
        for k, v in cfg.items():
            ae.set_config(k, v)
        ae.set_data(img, sch, mask, d.reshape(shape + (3,)))
        ae.set_model('FreeWater')
        ae.set_kernels(K, ht)
        return ae, ae.fit()
    ae, res = run(doSaveCorrectedDWI=True, doSavePredictedSignal=True, doComputeRMSE=True)
    assert list(res) == ['estimates', 'rmse', 'y_corrected', 'y_est'] and not calls
    corrected = ae.RESULTS['DWI_corrected']
    _check_evaluation(ae, res, img, sel, True, calls, True)
    # the error map of the same fit is the residual of the prediction
    assert np.abs(np.sqrt(np.mean((ae.y - res['y_est']) ** 2, axis=1)) - res['rmse']).max() < TOL
    # the corrected DWI is what the fit without the prediction makes, bit for bit, rows and volume; so are the maps
    ae0, res0 = run(doSaveCorrectedDWI=True, doComputeRMSE=True)
    assert 'y_est' not in res0 and 'DWI_predicted' not in ae0.RESULTS
    assert np.array_equal(ae0.RESULTS['DWI_corrected'], corrected) and np.array_equal(res0['y_corrected'], res['y_corrected'])
    assert np.array_equal(ae0.RESULTS['MAPs'], ae.RESULTS['MAPs']) and np.array_equal(res0['rmse'], res['rmse'])
    assert corrected[sel].any() and calls == [1]
