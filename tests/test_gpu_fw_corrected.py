"""Free-Water's corrected DWI from the fast fit: the isotropic coefficients as an output of every Free-Water kernel (AMX_F_FW_ISO), the
streaming kernel that makes the corrected rows / volume from them, Evaluation's route and FreeWaterVolumePipeline.
Every voxel is compared.  TOL is the bound tests/test_gpu_parity.py holds y_corrected to."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-6


# ------------------------------------------------------------------ shapes: one per kernel that writes Free-Water maps
# name: (b0 volumes, DWI volumes, zeppelins, d_isos, Mouse, float32 signals, lambda2, what ctx.last_path() must name)
SHAPES = {
    'fused11': (5, 60, 10, (2.5e-3,), False, True, 1e-3, 'k_freewater_fused<11>'),
    'fused12_mouse': (5, 60, 10, (1.5e-3, 3e-3), True, True, 1e-3, 'k_freewater_fused<12>'),
    'pair': (2, 40, 10, (2.5e-3,), False, True, 1e-3, 'k_fw_project_mfma -> k_freewater_refill'),
    'project_f64': (4, 96, 10, (2.5e-3,), False, False, 1e-3, 'k_fw_project -> k_freewater_refill'),
    'lane16': (5, 60, 14, (2.5e-3,), False, False, 1e-3, 'k_freewater_lane'),
    'wave20': (5, 60, 19, (2.5e-3,), False, False, 1e-3, 'wavefront per voxel'),
    'thin_qr': (5, 60, 10, (2.5e-3,), False, False, 0.0, 'wavefront per voxel'),
}


@functools.lru_cache(maxsize=None)
def _htable():
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'htable500.npz'), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def _case(name):
    """dictionary, the two signal sets and the oracle's answers for them: computed once on the CPU, shared, never modified.
    Set 0: 3 000 voxels with random directions.  Set 1: 2 500 voxels on two directions (1 250 each: more than one 1 024-voxel unit
    of the fused kernel and 64-voxel batches with a remainder; their signals keep the directions they were synthesised for, which
    is a valid fit all the same).  Each set must clip (y - fw < 0 somewhere): the clip is a branch of what is tested."""
    from amico_amd import synthetic as S
    from oracle import oracle
    n_b0, n_dwi, n_perp, d_isos, mouse, f32, lam2, _ = SHAPES[name]
    h = _htable()
    ht = h['htable']
    sch = S.make_scheme(n_b0, ((1000.0, n_dwi),), seed=3)
    K = S.freewater_kernels(sch, h['dirs'], d_perps=np.linspace(0.1, 1.0, n_perp) * 1e-3, d_isos=d_isos)
    csf = K['CSF'].astype(np.float64)
    sets = []
    for k, n in enumerate((3000, 2500)):
        for snr in (30.0, 20.0, 10.0, 5.0):
            y, d = S.freewater_signals(n, K, ht, sch, seed=11 + k, snr=snr)
            if k == 1:
                d = np.where(np.arange(n)[:, None] < n // 2, d[0], d[1])
            if f32:
                y = y.astype(np.float32)
            y64 = y.astype(np.float64)
            ref = oracle.freewater_fit(y64, d, K, ht, 0.0, lam2, is_mouse=mouse, corrected=True, nthreads=8, return_x=True)
            fw = ref['x'][:, n_perp:] @ csf
            if (y64 - fw < 0).any():
                break
        else:
            raise AssertionError('no signal set clips')
        assert ref['err'] == 0 and (ref['y_corrected'] == 0).any()
        sets.append((y, np.ascontiguousarray(d), ref))
    for y, d, ref in sets:
        for a in (ref['x'], ref['y_corrected'], ref['estimates']):
            a.setflags(write=False)
    return sch, K, sets


def _lut(ctx, K):
    from amico_amd import _capi
    return _capi.upload_freewater(ctx, K, _htable()['htable'])


def _restate(y64, x_iso, csf64):
    """models.pyx:1264-1274 elementwise, one rounding per operation, in the kernel's order"""
    fw = csf64[0][None, :] * x_iso[:, 0:1]
    for k in range(1, csf64.shape[0]):
        fw = fw + csf64[k][None, :] * x_iso[:, k:k + 1]
    yc = y64 - fw
    return np.where(yc < 0, 0.0, yc)


# ------------------------------------------------------------------ 1. x_iso of every route
@pytest.mark.parametrize('name', list(SHAPES))
def test_x_iso_of_every_freewater_kernel(name):
    import torch
    from amico_amd import _capi, get_context
    n_perp, mouse, lam2, path = SHAPES[name][2], SHAPES[name][4], SHAPES[name][6], SHAPES[name][7]
    sch, K, sets = _case(name)
    ctx = get_context()
    lut = _lut(ctx, K)
    for y, d, ref in sets:
        yt, dt = torch.from_numpy(y).cuda(), torch.from_numpy(d).cuda()
        est, _, _, _, xd, xi = _capi.freewater_fit_device(ctx, lut, yt, dt, 0.0, lam2, mouse, return_x=True, iso=True)
        ctx.sync()
        with_flag = ctx.last_path()
        est0 = _capi.freewater_fit_device(ctx, lut, yt, dt, 0.0, lam2, mouse)[0]
        ctx.sync()
        assert ctx.last_path() == with_flag and path in with_flag, with_flag
        x, x_iso = xd.cpu().numpy(), xi.cpu().numpy()
        assert x_iso.shape == (len(y), K['CSF'].shape[0])
        assert np.array_equal(x_iso, x[:, n_perp:])
        assert np.array_equal(est.cpu().numpy(), est0.cpu().numpy())
        worst = np.abs(x_iso - ref['x'][:, n_perp:]).max()
        print(f'{name}: {len(y)} voxels, max |x_iso - oracle| {worst:.3e}')
        assert worst < TOL
    # a voxel with a NaN sample: NaN coefficients, as its maps
    y, d, _ = sets[0]
    yn = y[:200].copy()
    yn[7, 3] = np.nan
    est, _, _, _, xi = _capi.freewater_fit_device(ctx, lut, torch.from_numpy(yn).cuda(), torch.from_numpy(d[:200].copy()).cuda(), 0.0, lam2,
                                                  mouse, iso=True)
    ctx.sync()
    x_iso, est = xi.cpu().numpy(), est.cpu().numpy()
    bad = np.arange(200) == 7
    assert np.isnan(x_iso[7]).all() and np.isnan(est[7]).all() and np.isfinite(x_iso[~bad]).all() and np.isfinite(est[~bad]).all()
    lut.close()


def test_fw_iso_flag_is_refused_without_buffer_and_on_other_models(noddi_fix):
    import torch
    from amico_amd import _capi, get_context
    sch, K, sets = _case('fused11')
    ctx = get_context()
    lut = _lut(ctx, K)
    y, d, _ = sets[0]
    yt, dt = torch.from_numpy(y[:64].copy()).cuda(), torch.from_numpy(d[:64].copy()).cuda()
    est = torch.empty((64, 3), dtype=torch.float64, device='cuda')
    L, p = _capi.lib(), _capi._dptr
    rc = L.amx_freewater_fit_device_f32(ctx._h, lut._h, p(yt), p(dt), 64, 0.0, 1e-3, 0, _capi.F_FW_ISO, p(est), None, None, None, None)
    assert rc == _capi.AMX_E_BADARG and b'amx_set_fw_iso' in L.amx_last_error(ctx._h)
    f = noddi_fix
    nl = _capi.upload_noddi(ctx, f['kernels'], _htable()['htable'], f['dwi_idx'])
    xi = torch.zeros((64, 1), dtype=torch.float64, device='cuda')
    ctx.check(L.amx_set_fw_iso(ctx._h, p(xi)))
    yn, dn = torch.from_numpy(f['y'][:64].copy()).cuda(), torch.from_numpy(f['dirs'][:64].copy()).cuda()
    rc = L.amx_noddi_fit_device(ctx._h, nl._h, p(yn), p(dn), 64, 0.5, 1e-3, _capi.F_FW_ISO, p(est), None, None, None, None)
    ctx.check(L.amx_set_fw_iso(ctx._h, None))
    assert rc == _capi.AMX_E_BADARG and b'FreeWater' in L.amx_last_error(ctx._h)
    ctx.sync()
    assert not xi.cpu().numpy().any()
    nl.close()
    lut.close()


def test_x_iso_of_a_voxel_skipped_for_its_direction_is_zero():
    """an out-of-bounds direction: the call reports it, the voxel's maps and coefficients are 0, everybody else's are written"""
    import torch
    from amico_amd import _capi, get_context
    sch, K, sets = _case('fused11')
    ctx = get_context()
    lut = _lut(ctx, K)
    y, d, _ = sets[0]
    db = d[:300].copy()
    db[5] = np.nan
    yt, dt = torch.from_numpy(y[:300].copy()).cuda(), torch.from_numpy(db).cuda()
    est = torch.full((300, 2), float('nan'), dtype=torch.float64, device='cuda')
    xi = torch.full((300, 1), float('nan'), dtype=torch.float64, device='cuda')
    L, p = _capi.lib(), _capi._dptr
    ctx.check(L.amx_set_fw_iso(ctx._h, p(xi)))
    ctx.check(L.amx_freewater_fit_device_f32(ctx._h, lut._h, p(yt), p(dt), 300, 0.0, 1e-3, 0, _capi.F_FW_ISO, p(est), None, None, None, None))
    ctx.check(L.amx_set_fw_iso(ctx._h, None))
    with pytest.raises(RuntimeError, match='index out of bounds'):
        ctx.sync()
    x_iso, est = xi.cpu().numpy(), est.cpu().numpy()
    ok = np.arange(300) != 5
    assert (x_iso[5] == 0).all() and (est[5] == 0).all() and np.isfinite(x_iso[ok]).all() and np.isfinite(est[ok]).all() and x_iso[ok].any()
    lut.close()


# ------------------------------------------------------------------ 2. rows form
@pytest.mark.parametrize('name', ['fused11', 'fused12_mouse', 'lane16'])
def test_corrected_rows_from_x_iso(name):
    """float32 input (one and two isotropic atoms) and float64 input (lane16).
    Against the rows AMX_F_CORRECTED writes for the same inputs the issue asks for "within 1e-12 relative".  Relative to the corrected
    value itself that cannot be held: next to the clip yc goes to 0 while the difference of two roundings of fw does not.  It is read
    here as relative to the sample, and tightened to what the arithmetic allows: the two results differ by the roundings of fw alone
    (that kernel may fuse its multiply-adds, this one rounds each product and sum), at most eps |fw| per isotropic atom with
    fw <= y wherever the result is not clipped to the same 0, plus the half ulp by which the final subtraction can then move: every
    element within 4 eps |y| = 8.9e-16 |y|.  Measured: 0 with one isotropic atom (float32 and float64 signals), 1.11e-16 with two."""
    import torch
    from amico_amd import _capi, get_context
    n_perp, mouse, lam2 = SHAPES[name][2], SHAPES[name][4], SHAPES[name][6]
    sch, K, sets = _case(name)
    csf64 = K['CSF'].astype(np.float64)
    ctx = get_context()
    lut = _lut(ctx, K)
    for y, d, ref in sets:
        yt, dt = torch.from_numpy(y).cuda(), torch.from_numpy(d).cuda()
        xi = _capi.freewater_fit_device(ctx, lut, yt, dt, 0.0, lam2, mouse, iso=True)[-1]
        rows = _capi.freewater_corrected_device(ctx, lut, yt, xi)
        today = _capi.freewater_fit_device(ctx, lut, yt, dt, 0.0, lam2, mouse, corrected=True)[3]
        ctx.sync()
        rows, today, x_iso = rows.cpu().numpy(), today.cpu().numpy(), xi.cpu().numpy()
        y64 = y.astype(np.float64)
        assert rows.dtype == np.float64 and rows.shape == y.shape
        assert np.array_equal(rows, _restate(y64, x_iso, csf64))
        assert (rows == 0).any()
        d_or, d_td = np.abs(rows - ref['y_corrected']).max(), np.abs(rows - today).max()
        print(f'{name}: max |rows - oracle| {d_or:.3e}, max |rows - AMX_F_CORRECTED| {d_td:.3e}')
        assert d_or < TOL
        assert (np.abs(rows - today) <= 4 * np.finfo(np.float64).eps * np.abs(y64)).all()
    lut.close()


# ------------------------------------------------------------------ 3. volume form, no fit involved
@pytest.mark.parametrize('n_iso', [1, 2])
@pytest.mark.parametrize('n_out', [7, 42, 65, 130])
@pytest.mark.parametrize('shape', [(13, 7, 5), (70, 3, 2)])
def test_corrected_volume_kernel(shape, n_out, n_iso):
    import torch
    from amico_amd import _capi, get_context, prep, synthetic as S
    h = _htable()
    n_b0 = 2 if n_out < 65 else 5
    sch = S.make_scheme(n_b0, ((1000.0, n_out - n_b0),), seed=1)
    K = S.freewater_kernels(sch, h['dirs'], d_perps=(0.5e-3,), d_isos=(2.5e-3, 1.2e-3)[:n_iso])
    csf64 = K['CSF'].astype(np.float64)
    ctx = get_context()
    lut = _capi.upload_freewater(ctx, K, h['htable'])
    rng = np.random.default_rng(n_out * 10 + n_iso)
    mask = (rng.uniform(size=shape) < 0.7).astype(np.uint8)
    mask[:, :, 0] = 0                                   # a slab without a masked voxel
    mask[2, 1, 1], mask[3, 1, 1], mask[4, 2, 1] = 1, 2, 1   # a 2 counts as unmasked
    sel = mask == 1
    n = int(sel.sum())
    # the plan is made from the MASK, as Evaluation makes it (its rule: mask == 1), for a Fortran-ordered image in the first shape (the
    # rank table is kept in the image's memory order) and a C-ordered one in the second
    img_like = np.zeros(shape + (n_out,), dtype=np.float32, order='F' if shape[0] == 13 else 'C')
    sp = prep.SignalPreparation(sch, img_like, mask, do_normalize=False, ctx=ctx)
    plan = sp._plan
    assert sp.n_vox == n
    y32 = rng.uniform(0.0, 1.2, (n, n_out)).astype(np.float32)
    x_iso = rng.uniform(0.0, 0.6, (n, n_iso))
    x_iso[3] = 50.0                                     # clipped entirely
    x_iso[5, -1] = np.nan
    mb0 = rng.uniform(300.0, 900.0, n).astype(np.float32)
    y64 = y32.astype(np.float64)
    yc = _restate(y64, x_iso, csf64)
    assert (yc[3] == 0).all() and (yc == 0).sum() > n_out and np.isnan(yc[5]).all()
    yt, xt, mt = torch.from_numpy(y32).cuda(), torch.from_numpy(x_iso).cuda(), torch.from_numpy(mb0).cuda()
    for rescale in (False, True):
        for keep in (False, True):
            m64 = mb0.astype(np.float64) if rescale else np.ones(n)
            exp_rows = (m64[:, None] * yc).astype(np.float32)
            if keep:
                exp_rows[:, sch.b0_idx] = (y64[:, sch.b0_idx] * m64[:, None]).astype(np.float32)
            exp = np.zeros(shape + (n_out,), dtype=np.float32)
            exp[sel] = exp_rows
            vol = torch.full(shape + (n_out,), float('nan'), dtype=torch.float32, device='cuda')
            plan.corrected_device(lut, yt, xt, vol, mt if rescale else None, sch.b0_idx if keep else ())
            ctx.sync()
            got = vol.cpu().numpy()
            assert np.array_equal(got, exp, equal_nan=True), (rescale, keep, int((got != exp).sum()))
            assert not got[~sel].any() and np.isnan(got[sel][5]).sum() == n_out - (n_b0 if keep else 0)
    lut.close()


# ------------------------------------------------------------------ 4. Evaluation
@pytest.mark.parametrize('keep_b0', [False, True])
@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('volumes', [(5, 60), (2, 40)])
def test_evaluation_corrected_dwi_stays_on_the_fast_fit(volumes, normalize, keep_b0):
    """the scene of tests/test_gpu_parity.py::test_evaluation_freewater_corrected_dwi, its assertions and tolerances"""
    import amico_amd
    from amico_amd import synthetic as S
    from oracle import oracle, signal_np
    h = _htable()
    ht = h['htable']
    sch = S.make_scheme(volumes[0], ((1000.0, volumes[1]),), seed=3)
    K = S.freewater_kernels(sch, h['dirs'])
    shape = (12, 10, 7)
    mask = np.ones(shape, dtype=np.uint8)
    mask[:, :, 0] = 0
    sel = mask == 1
    for snr in (30.0, 20.0, 10.0, 5.0):                 # (the scene's own SNR 30 clips nothing in these 840 voxels: lowered until it does)
        y, d = S.freewater_signals(int(np.prod(shape)), K, ht, sch, seed=2, snr=snr)
        img = (y.reshape(shape + (-1,)) * 640.0).astype(np.float32)
        y_ref, mb0 = signal_np.prepare_signal(img, mask, sch.b0_idx, sch.dwi_idx, do_normalize=normalize)
        d_ref = d.reshape(shape + (3,)).astype(np.float32)[sel].astype(np.float64)
        ref = oracle.freewater_fit(y_ref, d_ref, K, ht, corrected=True)
        if (ref['y_corrected'] == 0).any():
            break
    assert (ref['y_corrected'] == 0).any()
    ae = amico_amd.Evaluation()
    ae.set_config('doNormalizeSignal', normalize)
    ae.set_config('doSaveCorrectedDWI', True)
    ae.set_config('doKeepb0Intact', keep_b0)
    ae.set_data(img, sch, mask, d.reshape(shape + (3,)))
    ae.set_model('FreeWater')
    ae.set_kernels(K, ht)
    res = ae.fit()
    path = ae._prep.ctx.last_path()
    assert ('k_freewater_fused' if volumes[0] == 5 else 'k_freewater_refill') in path, path
    assert ae._y is None                                # the signals never came to the host
    assert np.abs(res['estimates'] - ref['estimates']).max() < 1e-6
    m = mb0[sel][:, None] if normalize else 1.0
    yc = ref['y_corrected'] * m
    if keep_b0:
        yc[:, sch.b0_idx] = y_ref[:, sch.b0_idx] * m
    vol = ae.RESULTS['DWI_corrected']
    assert vol.dtype == np.float32 and vol.shape == img.shape and not vol[:, :, 0].any()
    assert np.allclose(vol[sel], yc.astype(np.float32), rtol=1e-5, atol=1e-3)
    if keep_b0:
        assert np.allclose(vol[sel][:, sch.b0_idx], img[sel][:, sch.b0_idx], rtol=1e-6)      # b0 volumes intact
    assert 'y_corrected' in res and list(res) == ['estimates', 'y_corrected']
    rows = res['y_corrected']
    worst = np.abs(rows - ref['y_corrected']).max()
    print(f'{volumes} normalize={normalize}: max |y_corrected - oracle| {worst:.3e} at signal scale {np.abs(y_ref).max():.3g}')
    assert rows.dtype == np.float64 and rows.shape == (int(sel.sum()), sch.nS)
    assert worst < TOL
    assert ae._y is None


# ------------------------------------------------------------------ 5. pipeline
def test_freewater_volume_pipeline_equals_evaluation():
    import torch
    import amico_amd
    from amico_amd import pipeline, synthetic as S
    h = _htable()
    ht = h['htable']
    sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
    K = S.freewater_kernels(sch, h['dirs'])
    shape = (10, 8, 5)
    y, _ = S.freewater_signals(int(np.prod(shape)), K, ht, sch, seed=8)
    img = np.asfortranarray((y.reshape(shape + (-1,)) * 700.0).astype(np.float32))
    mask = np.random.default_rng(3).choice(np.array([0, 1, 1, 1, 2], dtype=np.uint8), size=shape)
    flat = np.lib.stride_tricks.as_strided(img, shape=(img.size,), strides=(4,))
    pl = pipeline.FreeWaterVolumePipeline(sch, img, mask, K, ht, corrected=True, keep_b0=True)
    maps, dirs = pl.run(torch.from_numpy(flat.copy()).to('cuda:0'))
    assert 'k_freewater_fused' in pl.ctx.last_path()
    ae = amico_amd.Evaluation()
    ae.set_config('doSaveCorrectedDWI', True)
    ae.set_config('doKeepb0Intact', True)
    ae.set_data(img, sch, mask)
    ae.set_model('FreeWater')
    ae.set_kernels(K, ht)
    ae.fit()
    assert maps.shape == shape + (2,) and pl.corrected.shape == img.shape
    assert np.array_equal(maps.cpu().numpy(), ae.RESULTS['MAPs']) and np.array_equal(dirs.cpu().numpy(), ae.RESULTS['DIRs'])
    corrected = pl.corrected.cpu().numpy()
    assert np.array_equal(corrected, ae.RESULTS['DWI_corrected']) and corrected[mask == 1].any() and not corrected[mask != 1].any()
    # without the switch nothing of it is made; b0_min_signal is Evaluation's, as for NODDI
    plain = pipeline.FreeWaterVolumePipeline(sch, img, mask, K, ht)
    maps0, _ = plain.run(torch.from_numpy(flat.copy()).to('cuda:0'))
    assert plain.corrected is None and np.array_equal(maps0.cpu().numpy(), maps.cpu().numpy())
    with pytest.raises(NotImplementedError):
        pipeline.FreeWaterVolumePipeline(sch, img, mask, K, ht, b0_min_signal=0.1)
    # one NaN in the image, replaced by the chain: what the chain gives for the image with a 0 there
    bad = flat.copy()
    pos = int(np.flatnonzero(mask.ravel(order='F') == 1)[4]) + 7 * int(np.prod(shape))      # volume 7 of a masked voxel (Fortran image)
    clean = bad.copy()
    bad[pos], clean[pos] = np.nan, 0.0
    pr = pipeline.FreeWaterVolumePipeline(sch, img, mask, K, ht, corrected=True, keep_b0=True, replace_bad_voxels=0.0)
    maps_r, _ = pr.run(torch.from_numpy(bad).to('cuda:0'))
    assert pr.bad_samples == 1 and pr.bad_samples_preprocessed == 0
    maps_c, _ = pl.run(torch.from_numpy(clean).to('cuda:0'))
    assert np.isfinite(pr.corrected.cpu().numpy()).all()
    assert np.array_equal(maps_r.cpu().numpy(), maps_c.cpu().numpy()) and np.array_equal(pr.corrected.cpu().numpy(), pl.corrected.cpu().numpy())
