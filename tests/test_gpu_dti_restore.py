"""The robust tensor fit on the GPU (DTI_fit_method 'RT' | 'RESTORE' | 'restore' with a sigma: amx_dti_create_robust,
amx_dti_fit_robust*) against its numpy restatement (tests/restore_np.py, pinned in tests/test_restore_np.py).

Bounds.  The outlier count is an integer: it has to EQUAL the restatement's, except where the restatement itself has a sample within
1e-4 sigma of the 3 sigma threshold (two correct implementations may put that sample on either side) or reached the trip cap; that share
is asserted to be <= 1 %.  Directions are held as test_dti_methods._nlls_check holds NLLS: the gap-weighted axis error against the
tight restatement at least 10 times below what MINPACK at dipy's default tolerances leaves on the same inlier sets, LUT indices
different in at most 1e-4 of the voxels.  Noise-free rows: axis within 1e-8 of the closed form, eigenvalues within EV_TOL of
test_gpu_dti_maps.py (relative to the largest |tensor entry|, which is below the largest eigenvalue used here).
"""
import numpy as np
import pytest

import amico_amd.synthetic as S
import dti_methods_np as M
import restore_np as R
from test_dti_methods import axis_error, lut_idx, rel_gap, well_separated
from test_gpu_dti_maps import EV_TOL, _scatter, _volume_scene
from test_restore_np import PLANTED_SIGMA, SIGMA, noisy_rows, planted_rows, scheme

pytestmark = pytest.mark.gpu

KEYS = ('directions', 'evals', 'scalars', 'outliers')


def _estimator(sc, sigma=SIGMA, method='RESTORE', **kw):
    from amico_amd import dti
    return dti.TensorDirections.from_scheme(sc, fit_method=method, **(dict(sigma=sigma, **kw) if sigma is not None else kw))


def _fit_device(est, y, f32, outliers=True):
    """the device entry points on rows of either type -> dict like fit_maps"""
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    d_y = torch.from_numpy(np.array(y, dtype=np.float32 if f32 else np.float64, order='C')).to(dev)
    n = y.shape[0]
    bufs = [torch.full((n, k), -7.0, dtype=torch.float64, device=dev) for k in (3, 3, 4)]
    d_out = torch.full((n,), -7, dtype=torch.int32, device=dev) if outliers else None
    est.fit_device(d_y.data_ptr(), n, bufs[0].data_ptr(), f32=f32, d_evals=bufs[1].data_ptr(), d_scalars=bufs[2].data_ptr(),
                   d_outliers=None if d_out is None else d_out.data_ptr())
    est.ctx.sync()
    got = dict(zip(KEYS, (b.cpu().numpy() for b in bufs)))
    if outliers:
        got['outliers'] = d_out.cpu().numpy()
    return got


# ----------------------------------------------------------------------------- 1. no outliers: NLLS, bit for bit
@pytest.mark.parametrize('f32', [False, True])
def test_huge_sigma_is_nlls(htable500, f32):
    sc, y = noisy_rows(htable500)
    if f32:
        y = y.astype(np.float32)
    rob, nl = _estimator(sc, sigma=1e30), _estimator(sc, sigma=None, method='NLLS')
    want = _fit_device(nl, y, f32, outliers=False)
    trips = nl._dti.last_trips()
    got = _fit_device(rob, y, f32)
    for key in KEYS[:3]:
        assert np.array_equal(got[key], want[key]), key
    assert got['outliers'].dtype == np.int32 and not got['outliers'].any()
    assert rob.last_robust() == (0, 0, 0, 0)
    assert rob._dti.last_trips() == trips and trips[0] > 0          # not one trip of step 3 or 4
    assert rob.last_unconverged() == 0
    if not f32:
        host = rob.fit_maps(y)
        assert sorted(host) == sorted(KEYS)
        for key in KEYS:
            assert np.array_equal(host[key], got[key]), key
        assert np.array_equal(rob.fit(y), want['directions'])
        assert nl.last_robust() == (0, 0, 0, 0) and 'outliers' not in nl.fit_maps(y[:3])


def test_outlier_counts_alone(htable500):
    """the outlier counts as the only output, host and device calls: the full call's counts, and nothing is written anywhere else"""
    import torch
    from amico_amd import _capi
    sc, y = noisy_rows(htable500)
    y = y[:130]
    est = _estimator(sc)
    full = _fit_device(est, y, False)
    assert full['outliers'].any()
    c, L = est.ctx, _capi.lib()
    host = np.full(len(y), -7, dtype=np.int32)
    c.check(L.amx_dti_fit_robust(c._h, est._dti._h, _capi._p(y, _capi.c_dp), len(y), est.min_diffusivity, None, None, None,
                                 _capi._p(host, _capi.c_i32p)))
    assert np.array_equal(host, full['outliers'])
    dev = torch.device('cuda', torch.cuda.current_device())
    for f32 in (False, True):
        d_y = torch.from_numpy(np.array(y, dtype=np.float32 if f32 else np.float64, order='C')).to(dev)
        d_out = torch.full((len(y),), -7, dtype=torch.int32, device=dev)
        est.fit_device(d_y.data_ptr(), len(y), None, f32=f32, d_outliers=d_out.data_ptr())
        c.sync()
        assert np.array_equal(d_out.cpu().numpy(), full['outliers']), f32
        # counts and directions, no maps: the direction kernel's variant
        d_dirs = torch.zeros((len(y), 3), dtype=torch.float64, device=dev)
        d_out.fill_(-7)
        est.fit_device(d_y.data_ptr(), len(y), d_dirs.data_ptr(), f32=f32, d_outliers=d_out.data_ptr())
        c.sync()
        assert np.array_equal(d_out.cpu().numpy(), full['outliers']) and np.array_equal(d_dirs.cpu().numpy(), full['directions'])
    # no output at all stays the refusal it was, and the counts belong to a robust estimator
    with pytest.raises(ValueError, match='amx_dti_directions: null buffer'):
        est._dti.fit_device(d_y.data_ptr(), len(y), est.min_diffusivity, None, None, None, f32=True)
    with pytest.raises(ValueError, match='d_outliers belongs to a RESTORE estimator'):
        _estimator(sc, sigma=None, method='NLLS').fit_device(d_y.data_ptr(), len(y), d_dirs.data_ptr(), f32=True, d_outliers=d_out.data_ptr())


# ----------------------------------------------------------------------------- 2. planted outliers, noise-free
@pytest.mark.parametrize('n_vol', [33, 99])
def test_planted_outliers_noise_free(n_vol):
    sc = scheme(n_vol)
    y, axis, evals, planted = planted_rows(sc, 24, seed=n_vol)
    est = _estimator(sc, sigma=PLANTED_SIGMA)
    got = est.fit_maps(y)
    e_axis = axis_error(got['directions'], axis).max()
    e_ev = (np.abs(got['evals'] - evals) / evals[:, :1]).max()
    print('%d volumes: axis %.3g, eigenvalues %.3g, counters %s, trips %s' % (n_vol, e_axis, e_ev, est.last_robust(), est._dti.last_trips()))
    assert np.array_equal(got['outliers'], planted.sum(1))
    assert est.last_robust() == (24, 24, 0, 0) and est.last_unconverged() == 0
    assert e_axis < 1e-8
    assert e_ev <= EV_TOL
    nl = _estimator(sc, sigma=None, method='NLLS').fit(y)
    assert np.median(axis_error(nl, axis)) > 1e-2                    # (the plain fit is off by degrees on these rows)


# ----------------------------------------------------------------------------- 3. noisy rows with planted outliers
@pytest.fixture(scope='module')
def noisy_reference(htable500):
    sc, y = noisy_rows(htable500)
    X = M.design(sc.b, sc.raw[:, :3])
    ref = R.restore(y, X, SIGMA)
    ref['default'] = R.refit_default(y, X, ref['mask'])
    return sc, y, ref


@pytest.mark.parametrize('f32', [False, True])
def test_noisy_rows_vs_restatement(htable500, noisy_reference, f32):
    sc, y, ref = noisy_reference
    if f32:                                                          # (the rows of noddi_signals are float32 values: the same numbers)
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    est = _estimator(sc)
    got = _fit_device(est, y, f32)
    counters, trips = est.last_robust(), est._dti.last_trips()
    keep = (ref['margin'] >= 1e-4) & ~ref['capped']
    print('restatement: entered %d refitted %d capped %d, margin min %.3g; device counters %s trips %s; kept %d of %d'
          % (ref['entered'].sum(), ref['refitted'].sum(), ref['capped'].sum(), ref['margin'].min(), counters, trips, keep.sum(), len(y)))
    assert (~keep).mean() <= 0.01
    assert np.array_equal(got['outliers'][keep], ref['outliers'][keep])
    # the counters: the restatement's, give or take the voxels that are not compared
    slack = int((~keep).sum())
    for got_count, name in zip(counters, ('entered', 'refitted', 'capped', 'few')):
        assert abs(got_count - int(ref[name].sum())) <= slack, (name, got_count, int(ref[name].sum()), slack)
    assert est.last_unconverged() == 0
    # directions: the project's NLLS rule on the inlier sets
    tight, ev = M.decompose(ref['params'])
    default, _ = M.decompose(ref['default'])
    separated = well_separated(ev)
    assert separated.mean() >= 0.999                                 # (_nlls_check's share, before the uncompared voxels are taken out)
    ok = separated & keep
    gap = rel_gap(ev)[ok]
    e_dev = (axis_error(got['directions'][ok], tight[ok]) * gap).max()
    e_def = (axis_error(default[ok], tight[ok]) * gap).max()
    print('gap-weighted axis error: device %.3g, MINPACK default %.3g (plain %.3g / %.3g), %d voxels'
          % (e_dev, e_def, axis_error(got['directions'][ok], tight[ok]).max(), axis_error(default[ok], tight[ok]).max(), ok.sum()))
    assert np.allclose(np.linalg.norm(got['directions'], axis=1), 1.0, atol=1e-12)
    assert 10.0 * e_dev <= e_def, (e_dev, e_def)
    differ = (lut_idx(tight[ok], htable500['htable']) != lut_idx(got['directions'][ok], htable500['htable'])).mean()
    assert differ <= 1e-4, differ
    # and the outliers matter: plain NLLS has other axes
    nl = _estimator(sc, sigma=None, method='NLLS').fit(y)
    assert np.median(axis_error(nl[ref['refitted']], got['directions'][ref['refitted']])) > 1e-3


# ----------------------------------------------------------------------------- 4. shapes
COUNTS = (1, 7, 63, 65, 257)


@pytest.mark.parametrize('n_vol', [8, 33, 99, 130, 288, 512])
def test_shapes(n_vol):
    """every tile length and the ragged ends of tiles and of the eight-lane groups: a voxel's fit does not depend on its tile; clean and
    corrupted voxels alternate, so every wavefront holds voxels that stop at step 2 beside voxels that go on"""
    sc = scheme(n_vol)
    # (8 volumes: 7 parameters absorb a mild outlier; +1.5 sends a share of the voxels round step 3 until its cap -- 6 of the 84 that
    #  enter it on this scene in the restatement, see tests/test_restore_np.py::test_cap_is_a_path_at_8_volumes -- and leaves 3 of
    #  them fewer than 7 inliers)
    y, axis, _, planted = planted_rows(sc, COUNTS[-1], seed=100 + n_vol, every=2, amp=1.5 if n_vol == 8 else 0.5)
    y = np.abs(y + np.random.default_rng(n_vol).normal(scale=SIGMA, size=y.shape))
    est = _estimator(sc)
    full = _fit_device(est, y, False)
    counters, out = est.last_robust(), full['outliers']
    print('%d volumes: counters %s, unconverged %d, trips %s, outliers max %d' % (n_vol, counters, est.last_unconverged(),
                                                                                est._dti.last_trips(), out.max()))
    for key in KEYS:
        assert np.isfinite(full[key]).all(), key
    assert (out >= 0).all() and (out <= n_vol).all()
    entered, refitted, capped, few = counters
    assert refitted == ((out > 0) & (out <= n_vol - 7)).sum()        # a refit leaves at least 7 samples in
    assert few == (out > n_vol - 7).sum()
    assert entered >= refitted + few and capped <= entered <= len(y)
    if n_vol == 8:
        assert capped > 0                                            # the cap is a path that ran
    else:
        corrupted = planted.any(1)
        assert (out[corrupted] >= planted.sum(1)[corrupted]).all()   # +0.5 is 15 sigma: found, beside what the noise adds
        assert entered >= corrupted.sum() and capped == 0 and few == 0
        assert np.median(axis_error(full['directions'][corrupted], axis[corrupted])) < 0.2
    for n in COUNTS[:-1]:
        part = _fit_device(est, y[:n], False)
        for key in KEYS:
            assert np.array_equal(part[key], full[key][:n]), (n, key)
    assert np.array_equal(_fit_device(est, y[:65].astype(np.float32), True)['outliers'],
                          _fit_device(est, y[:65].astype(np.float32).astype(np.float64), False)['outliers'])


def test_too_long_a_scheme_is_refused():
    sc = S.make_scheme(n_b0=8, shells=((1000.0, 512),), seed=1)
    est = _estimator(sc)
    with pytest.raises(ValueError, match='scheme too long'):
        est.fit(np.ones((4, sc.nS)))


# ----------------------------------------------------------------------------- 5. odd samples
@pytest.mark.parametrize('f32', [False, True])
def test_odd_samples(htable500, f32):
    """what include/amico_amd.h documents for NLLS holds here: a NaN and a sample below min_signal count as min_signal, a +Inf sample
    leaves NaN eigenvalues and scalars and no outlier; the other voxels of the tiles keep their bits"""
    sc, y = noisy_rows(htable500)
    y = y[:192]
    est = _estimator(sc)
    clean = _fit_device(est, y, f32)
    bad = y.copy()
    bad[5] = 0.0
    bad[70, 40] = 1e-6
    bad[131, 17] = np.nan
    bad[150, 3] = np.inf
    got = _fit_device(est, bad, f32)
    as_clipped = bad[[70, 131]].copy()
    as_clipped[0, 40] = as_clipped[1, 17] = est.min_signal
    one = _fit_device(est, as_clipped, f32)
    for key in KEYS:
        assert np.isfinite(got[key][[5, 70, 131]]).all(), key
        assert np.array_equal(got[key][[70, 131]], one[key]), key
    assert got['outliers'][5] == 0
    assert np.isnan(got['evals'][150]).all() and np.isnan(got['scalars'][150]).all() and got['outliers'][150] == 0
    rest = np.ones(len(y), dtype=bool)
    rest[[5, 70, 131, 150]] = False
    for key in KEYS:
        assert np.array_equal(got[key][rest], clean[key][rest]), key


# ----------------------------------------------------------------------------- 6. Evaluation
def _corrupt(scene, seed=3):
    """+0.6 b0 on 4 random volumes of every other voxel or so -> (the scene with that image, which voxels)"""
    sch, K, ht, img, mask, d = scene
    img = img.copy(order='F')
    rng = np.random.default_rng(seed)
    b0 = img[..., sch.b0_idx].mean(-1)
    hit = rng.uniform(size=img.shape[:3]) < 0.5
    for idx in zip(*np.nonzero(hit)):
        img[idx][rng.choice(sch.nS, 4, replace=False)] += 0.6 * b0[idx]
    return (sch, K, ht, img, mask, d), hit


def _evaluate(scene, model, **config):
    import amico_amd
    sch, K, ht, img, mask, _ = scene
    ae = amico_amd.Evaluation()
    for key, value in config.items():
        ae.set_config(key.replace('DWI_SNR', 'DWI-SNR'), value)
    ae.set_data(img, sch, mask)
    ae.set_model(model)
    ae.set_kernels(K, ht)
    return ae, ae.fit()


@pytest.mark.parametrize('model', ['NODDI', 'FreeWater'])
def test_evaluation(htable500, model):
    from amico_amd import dti
    snr = 30.0 if model == 'NODDI' else 20.0
    scene, hit = _corrupt(_volume_scene(htable500, model))
    sch, K, ht, img, mask, _ = scene
    sel = mask == 1
    a, res = _evaluate(scene, model, DTI_fit_method='RESTORE', DTI_sigma=1.0 / snr, doSaveTensorMaps=True)
    b, _ = _evaluate(scene, model, DTI_fit_method='restore', DWI_SNR=snr, doSaveTensorMaps=True)
    new = ['DTI_MAPs', 'DTI_evals', 'DTI_outliers']
    if model == 'FreeWater':
        new += [k + '_corrected' for k in new]
    assert sorted(a.RESULTS) == sorted(b.RESULTS) == sorted(['DIRs', 'MAPs'] + new)
    for key in a.RESULTS:
        assert a.RESULTS[key].tobytes() == b.RESULTS[key].tobytes(), key
    est = dti.TensorDirections.from_scheme(sch, fit_method='RT', sigma=1.0 / snr)
    same = _fit_device(est, a.y, True)                   # the call fit() makes: float32 rows in HBM
    assert np.array_equal(a.RESULTS['DIRs'], _scatter(same['directions'], sel))
    assert np.array_equal(a.RESULTS['DIRs'][sel], est.fit(a.y).astype(np.float32))
    assert np.array_equal(a.RESULTS['DTI_evals'], _scatter(same['evals'], sel))
    vol = a.RESULTS['DTI_outliers']
    assert vol.dtype == np.float32 and vol.shape == mask.shape and not vol[~sel].any()
    assert np.array_equal(vol[sel], same['outliers'].astype(np.float32))
    # the planted samples are found: 4 more outliers per corrupted voxel than per clean one, give or take one (a two-shell signal is no
    # single tensor's, so at SNR 30 the verdict also leaves out samples that the tensor model misses, in both kinds of voxel alike)
    print('%s: outliers per voxel, corrupted %.2f, clean %.2f, max %d' % (model, vol[sel & hit].mean(), vol[sel & ~hit].mean(), vol.max()))
    assert 3.0 <= vol[sel & hit].mean() - vol[sel & ~hit].mean() <= 5.0
    counters = a.get_config('dti_robust')
    assert counters == est.last_robust() and counters[0] >= (vol[sel] > 0).sum() and counters[1] == (vol[sel] > 0).sum()
    plain, _ = _evaluate(scene, model, DTI_fit_method='NLLS')
    assert np.median(axis_error(plain.RESULTS['DIRs'][sel].astype(float), a.RESULTS['DIRs'][sel].astype(float))) > 1e-3
    # without the maps: the same directions, nothing else
    c, _ = _evaluate(scene, model, DTI_fit_method='RESTORE', DWI_SNR=snr)
    assert sorted(c.RESULTS) == ['DIRs', 'MAPs'] and c.RESULTS['DIRs'].tobytes() == a.RESULTS['DIRs'].tobytes()
    assert c.get_config('dti_robust') == counters
    if model == 'FreeWater':
        again = est.fit_maps(res['y_corrected'])
        vol = a.RESULTS['DTI_outliers_corrected']
        assert vol.dtype == np.float32 and not vol[~sel].any()
        assert np.array_equal(vol[sel], again['outliers'].astype(np.float32))
        assert np.array_equal(a.RESULTS['DTI_evals_corrected'], _scatter(again['evals'], sel))
    # no sigma to be had: the refusal of always, raised where the tensor fit would run
    for config in (dict(), dict(DWI_SNR=snr, doNormalizeSignal=False)):
        with pytest.raises(NotImplementedError, match='sigma'):
            _evaluate(scene, model, DTI_fit_method='RESTORE', **config)


# ----------------------------------------------------------------------------- 7. fused gather
def test_gather_with_directions_takes_the_two_kernel_route():
    """amx_prep_gather_directions_device_f32 with a RESTORE handle = gather + amx_dti_directions_device_f32, bit for bit"""
    import torch
    from amico_amd import prep, dti, _capi
    sc = S.make_scheme()
    rng = np.random.default_rng(3)
    shape = (30, 9, 5)
    img = rng.uniform(50.0, 900.0, shape + (sc.nS,)).astype(np.float32)
    img[..., sc.b0_idx] += 600.0
    mask = (rng.uniform(size=shape) < 0.6).astype(np.uint8)
    sp = prep.SignalPreparation(sc, img, mask)
    td = dti.TensorDirections.from_scheme(sc, ctx=sp.ctx, fit_method='RESTORE', sigma=0.12)
    L, c = _capi.lib(), sp.ctx
    dev = torch.device('cuda', 0)
    d_img = torch.from_numpy(np.lib.stride_tricks.as_strided(img, shape=(img.size,), strides=(4,)).copy()).to(dev)
    n, m = sp.n_vox, sp.n_out
    y_a, y_b = torch.zeros((n, m), dtype=torch.float32, device=dev), torch.zeros((n, m), dtype=torch.float32, device=dev)
    mb_a, mb_b = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    d_a, d_b = torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros((n, 3), dtype=torch.float64, device=dev)
    norm = int(sp.do_normalize)
    c.check(L.amx_prep_gather_device_f32(c._h, sp._plan._h, d_img.data_ptr(), norm, 0.0, y_a.data_ptr(), mb_a.data_ptr(), None))
    td.fit_device(y_a.data_ptr(), n, d_a.data_ptr(), None, f32=True)
    first = td.last_robust()
    c.check(L.amx_prep_gather_directions_device_f32(c._h, sp._plan._h, td._dti._h, d_img.data_ptr(), norm, 0.0, y_b.data_ptr(),
                                                    mb_b.data_ptr(), d_b.data_ptr(), None))
    c.sync(None)
    assert torch.equal(y_a, y_b) and torch.equal(mb_a, mb_b)
    assert n > 500 and torch.isfinite(d_a).all() and torch.equal(d_a, d_b)
    assert td.last_robust() == first and first[0] > 0                # (uniform noise, much of it beyond 3 sigma: the robust path ran)
    nl = dti.TensorDirections.from_scheme(sc, ctx=sp.ctx, fit_method='NLLS').fit(y_a.cpu().numpy().astype(np.float64))
    assert np.median(axis_error(d_a.cpu().numpy(), nl)) > 1e-4
