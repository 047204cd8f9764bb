"""Principal directions with DTI_fit_method 'WLS' and 'NLLS' (core.py:419-420, 436 of the reference): the numpy restatement of
dipy's routines (tests/dti_methods_np.py) against an independent route, and the HIP kernels against the restatement.

Yardsticks of the GPU tests are those of tests/test_signal.py::test_dti_directions_vs_oracle_synthetic: over the voxels whose
principal axis is defined (`well_separated`), sine of the angle between the axes < 1e-8, the same times the relative
eigenvalue gap < 1e-12, and the LUT index (what the fit consumes) different in at most 1e-4 of the voxels.  NLLS is only
defined to the reference's stopping rule, so its bound is computed by the test itself: the device has to be at least 10 times
closer to MINPACK run to ftol = xtol = 1e-15 than MINPACK at dipy's default tolerances is.
"""
import numpy as np
import pytest

import amico_amd.synthetic as S
from conftest import load_npz
from oracle import signal_np
import dti_methods_np as M


def axis_error(a, b):
    """sine of the angle between two axes (eigenvectors have no defined sign)"""
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.linalg.norm(np.cross(a, b), axis=1)


def well_separated(evals, rel=1e-6, absolute=1e-9):
    gap = evals[:, 0] - evals[:, 1]
    return (gap > rel * np.abs(evals[:, 0])) & (gap > absolute)


def rel_gap(evals):
    return (evals[:, 0] - evals[:, 1]) / np.abs(evals[:, 0])


def lut_idx(dirs, htable):
    from oracle import oracle
    return oracle.dir_to_lut_idx(np.ascontiguousarray(dirs), htable)[0]


@pytest.fixture(scope='module')
def dti_fix():
    f = load_npz('dti_fixture.npz')
    f.update(load_npz('dti_methods_fixture.npz'))
    return f


@pytest.fixture(scope='module')
def noddi_setup(htable500):
    sc = S.make_scheme()
    return sc, S.noddi_kernels(sc, htable500['dirs'])


# ----------------------------------------------------------------------------- CPU: restatement vs independent route
def test_restatement_vs_golden(dti_fix):
    """wls_params / nlls_params against scipy's gelsd on the weighted system and scipy.optimize.least_squares (no shared code)"""
    sc = dti_fix['scheme']
    X = M.design(sc[:, 3], sc[:, :3])
    p_wls = M.wls_params(dti_fix['y'], X)
    scale = np.abs(dti_fix['p_wls']).max(axis=1, keepdims=True)
    assert (np.abs(p_wls - dti_fix['p_wls']) / scale).max() < 1e-10
    p_nl = M.nlls_params(dti_fix['y'], X, tight=True)
    scale = np.abs(dti_fix['p_nlls']).max(axis=1, keepdims=True)
    # two optimisers at the same minimum: each is converged to ~sqrt(eps) in the parameters where the residual is not zero
    assert (np.abs(p_nl - dti_fix['p_nlls']) / scale).max() < 1e-6
    d_a, ev = M.decompose(p_nl)
    d_b, _ = M.decompose(dti_fix['p_nlls'])
    ok = well_separated(ev)
    assert ok.sum() > 200 and (axis_error(d_a[ok], d_b[ok]) * rel_gap(ev)[ok]).max() < 1e-6


@pytest.mark.parametrize('method', ['OLS', 'WLS', 'NLLS'])
def test_restatement_closed_form(dti_fix, method):
    """noise-free single-tensor voxels: the log-signal is linear in the parameters, so every method is exact"""
    sc = dti_fix['scheme']
    dirs = M.directions(dti_fix['y'][160:], sc[:, 3], sc[:, :3], method, tight=True)
    assert axis_error(dirs, dti_fix['closed_form_axis']).max() < 1e-10


def test_method_names_and_arguments(monkeypatch):
    """host-side rules: they are checked before a context or a device is needed"""
    from amico_amd import dti, _capi
    b = np.array([0.0] + [1000.0] * 7)
    g = np.vstack([np.zeros(3), np.eye(3), np.array([[1, 1, 0], [1, 0, 1], [0, 1, 1], [1, -1, 0]]) / np.sqrt(2)])
    with pytest.raises(ValueError, match="'WLS': weighted least squares"):
        dti.TensorDirections(b, g, fit_method='wls')
    with pytest.raises(ValueError, match='DTI fit method must be one of the following'):
        dti.TensorDirections(b, g, fit_method=None)
    for name in ('RT', 'RESTORE', 'restore'):
        with pytest.raises(NotImplementedError, match='sigma'):
            dti.TensorDirections(b, g, fit_method=name)
    assert dti.FIT_METHODS == {'OLS': 'OLS', 'LS': 'OLS', 'WLS': 'WLS', 'NLLS': 'NLLS'}
    for name in ('OLS', 'LS', 'WLS', 'NLLS', 'RT', 'RESTORE', 'restore'):
        dti.check_fit_method(name)
    w = np.zeros((7, 8))
    with pytest.raises(ValueError, match='needs the design matrix'):
        _capi.Dti(None, w, method='WLS')
    with pytest.raises(ValueError, match=r'shape \[nS, 7\]'):
        _capi.Dti(None, w, design=np.zeros((7, 8)), method='NLLS')
    with pytest.raises(ValueError, match='method must be one of'):
        _capi.Dti(None, w, design=np.zeros((8, 7)), method='LS')
    with pytest.raises(ValueError, match='inv_design'):
        _capi.Dti(None, np.zeros((8, 7)), design=np.zeros((8, 7)), method='WLS')


def test_evaluation_rejects_unknown_method_before_upload():
    """the name check sits where the reference has it (core.py:419): nothing has touched the device yet"""
    import amico_amd
    sc = S.make_scheme()
    ae = amico_amd.Evaluation()
    ae.niiDWI_img = np.zeros((2, 2, 2, sc.nS), dtype=np.float32)
    ae.model = type('M', (), {'id': 'NODDI', 'name': 'NODDI'})()
    ae.KERNELS = {'model': 'NODDI'}
    ae.set_config('DTI_fit_method', 'GLS')
    with pytest.raises(ValueError, match='DTI fit method must be one of the following'):
        ae.fit()


# ----------------------------------------------------------------------------- GPU
def _check_vs_ref(dirs, ref, evals, htable, min_share=0.999):
    ok = well_separated(evals)
    assert ok.mean() >= min_share, ok.mean()
    err = axis_error(dirs[ok], ref[ok])
    gap = rel_gap(evals)[ok]
    print('axis error max %.3g, gap-weighted max %.3g over %d voxels' % (err.max(), (err * gap).max(), ok.sum()))
    assert np.allclose(np.linalg.norm(dirs, axis=1), 1.0, atol=1e-12)
    assert err.max() < 1e-8 and (err * gap).max() < 1e-12
    differ = (lut_idx(ref[ok], htable) != lut_idx(dirs[ok], htable)).mean()
    assert differ <= 1e-4, differ


@pytest.mark.gpu
def test_wls_golden(dti_fix, htable500):
    from amico_amd import dti
    sc = dti_fix['scheme']
    ref, ev = M.decompose(dti_fix['p_wls'])
    dirs = dti.TensorDirections(sc[:, 3], sc[:, :3], fit_method='WLS').fit(dti_fix['y'])
    ok = well_separated(ev)
    assert ok.sum() > 200
    assert axis_error(dirs[ok], ref[ok]).max() < 1e-8
    assert axis_error(dirs[160:], dti_fix['closed_form_axis']).max() < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('n_vox', [1, 63, 64, 65, 20011])
def test_wls_vs_restatement_synthetic(htable500, noddi_setup, n_vox, f32):
    import torch
    from amico_amd import dti
    sc, K = noddi_setup
    y, _ = S.noddi_signals(n_vox, K, htable500['htable'], sc, seed=5)
    est = dti.TensorDirections.from_scheme(sc, fit_method='WLS')
    if f32:
        y = y.astype(np.float32)
        dirs = _fit_device_f32(est, y)
        y = y.astype(np.float64)
    else:
        dirs = est.fit(y)
    ref, ev = M.directions(y, sc.b, sc.raw[:, :3], 'WLS', return_evals=True)
    if n_vox < 1000:                        # (a share of 99.9 % says nothing about a handful of voxels)
        assert well_separated(ev).all()
    _check_vs_ref(dirs, ref, ev, htable500['htable'])


def _fit_device_f32(est, y32):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    d_y = torch.from_numpy(np.ascontiguousarray(y32, dtype=np.float32)).to(dev)
    d_dirs = torch.zeros((y32.shape[0], 3), dtype=torch.float64, device=dev)
    est.fit_device(d_y.data_ptr(), y32.shape[0], d_dirs.data_ptr(), f32=True)
    est.ctx.sync()
    return d_dirs.cpu().numpy()


def _nlls_check(est, y, bvals, bvecs, htable, dirs, label, min_share=0.999):
    """the mandatory NLLS criterion: max over the well-separated voxels of the gap-weighted axis error against MINPACK run to
    1e-15 (`ref_tight`), at least 10 times below what MINPACK at dipy's default tolerances (`ref_default`) leaves"""
    X = M.design(bvals, bvecs)
    tight, ev = M.decompose(M.nlls_params(y, X, tight=True))
    default, _ = M.decompose(M.nlls_params(y, X))
    ok = well_separated(ev)
    assert ok.mean() >= min_share, ok.mean()
    gap = rel_gap(ev)[ok]
    e_dev = (axis_error(dirs[ok], tight[ok]) * gap).max()
    e_def = (axis_error(default[ok], tight[ok]) * gap).max()
    print('%s: gap-weighted axis error device %.3g, MINPACK default %.3g (plain: %.3g / %.3g), %d voxels'
          % (label, e_dev, e_def, axis_error(dirs[ok], tight[ok]).max(), axis_error(default[ok], tight[ok]).max(), ok.sum()))
    assert np.allclose(np.linalg.norm(dirs, axis=1), 1.0, atol=1e-12)
    assert 10.0 * e_dev <= e_def, (e_dev, e_def)
    differ = (lut_idx(tight[ok], htable) != lut_idx(dirs[ok], htable)).mean()
    assert differ <= 1e-4, differ
    assert est.last_unconverged() == 0


@pytest.mark.gpu
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('n_vox', [1, 63, 64, 65, 600])
def test_nlls_vs_minpack_synthetic(htable500, noddi_setup, n_vox, f32):
    """measured on an MI355X (600 voxels, float64 / float32 signals): see DESIGN.md, "WLS and NLLS directions" """
    from amico_amd import dti
    sc, K = noddi_setup
    y, _ = S.noddi_signals(600, K, htable500['htable'], sc, seed=5)
    est = dti.TensorDirections.from_scheme(sc, fit_method='NLLS')
    if f32:
        y = y.astype(np.float32)
        dirs = _fit_device_f32(est, y[:n_vox])
        y = y.astype(np.float64)
    else:
        dirs = est.fit(y[:n_vox])
    assert est.last_unconverged() == 0
    if n_vox < 600:
        # ragged tiles: the same voxels as the head of the full call, bit for bit (a voxel's fit does not depend on its tile)
        full = est.fit(y)
        assert np.array_equal(full[:n_vox], dirs)
        return
    _nlls_check(est, y, sc.b, sc.raw[:, :3], htable500['htable'], dirs, 'noddi_signals f32=%s' % f32)


@pytest.mark.gpu
def test_nlls_golden(dti_fix, htable500):
    from amico_amd import dti
    sc = dti_fix['scheme']
    est = dti.TensorDirections(sc[:, 3], sc[:, :3], fit_method='NLLS')
    dirs = est.fit(dti_fix['y'])
    assert est.last_unconverged() == 0
    assert axis_error(dirs[160:], dti_fix['closed_form_axis']).max() < 1e-10
    # the noisy voxels against scipy.optimize.least_squares (the fixture's independent route) ...
    ref, ev = M.decompose(dti_fix['p_nlls'])
    ok = well_separated(ev)
    ok[160:] = False
    assert (axis_error(dirs[ok], ref[ok]) * rel_gap(ev)[ok]).max() < 1e-6
    # ... and by the criterion of the synthetic test (the fixture holds a few all-zero / isotropic voxels on purpose)
    _nlls_check(est, dti_fix['y'][:160], sc[:, 3], sc[:, :3], htable500['htable'], dirs[:160], 'fixture', min_share=0.95)


def _single_tensor(sc, merge, n=130):
    rng = np.random.default_rng(1)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    D = (q * np.array([1.7e-3, 0.4e-3, 0.3e-3])) @ q.T
    b, g = sc.b, sc.raw[:, :3]
    y = np.exp(-b * np.einsum('ij,jk,ik->i', g, D, g))[None, :].repeat(n, 0)
    if merge:
        y = np.hstack([y[:, sc.b0_idx].mean(1, keepdims=True), y[:, sc.dwi_idx]])
    return y, q[:, 0][None, :].repeat(n, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['WLS', 'NLLS'])
def test_other_schemes_and_merge_b0(method):
    """the two cases of test_dti_other_schemes_and_merge_b0 (single shell 64 directions + 1 b0; three shells with doMergeB0)
    and the shortest scheme amx_dti_create admits (7 volumes: the fit interpolates)"""
    from amico_amd import dti
    for sc, merge in ((S.make_scheme(n_b0=1, shells=((1000.0, 64),), seed=2), False),
                      (S.make_scheme(n_b0=6, shells=((1000.0, 20), (2000.0, 30), (3000.0, 94)), seed=3), True),
                      (S.make_scheme(n_b0=1, shells=((1000.0, 6),), seed=4), False)):
        y, axis = _single_tensor(sc, merge)
        est = dti.TensorDirections.from_scheme(sc, do_merge_b0=merge, fit_method=method)
        d = est.fit(y)
        assert axis_error(d, axis).max() < 1e-10, (sc.nS, merge)
        assert est.last_unconverged() == 0


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['WLS', 'NLLS'])
def test_degenerate_voxels(htable500, noddi_setup, method):
    from amico_amd import dti
    sc, K = noddi_setup
    y, _ = S.noddi_signals(192, K, htable500['htable'], sc, seed=9)
    est = dti.TensorDirections.from_scheme(sc, fit_method=method)
    clean = est.fit(y)
    bad = y.copy()
    bad[5] = 0.0                    # all zeros
    bad[70] = 1e-6                  # all below min_signal
    bad[131, 17] = np.nan           # one NaN volume
    d = est.fit(bad)
    for i in (5, 70):
        assert np.isfinite(d[i]).all() and abs(np.linalg.norm(d[i]) - 1.0) < 1e-12
    rest = np.ones(len(y), dtype=bool)
    rest[[5, 70, 131]] = False
    assert np.array_equal(d[rest], clean[rest])           # the other voxels of the tiles are untouched
    ols = dti.TensorDirections.from_scheme(sc).fit(bad)
    assert np.isfinite(d[131]).all() == np.isfinite(ols[131]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['WLS', 'NLLS'])
@pytest.mark.parametrize('f32', [False, True])
def test_amplitude(htable500, noddi_setup, method, f32):
    """the weights of WLS scale with the signal and the cost of NLLS with its square; the directions do not (min_signal is
    scaled along, so that the same samples are clipped): same LUT index as at unit scale from 2^-10 to 2^14"""
    from amico_amd import dti
    sc, K = noddi_setup
    y, _ = S.noddi_signals(2000, K, htable500['htable'], sc, seed=11)
    if f32:
        y = y.astype(np.float32)
    fit = (lambda e, v: _fit_device_f32(e, v)) if f32 else (lambda e, v: e.fit(v))
    base = fit(dti.TensorDirections.from_scheme(sc, fit_method=method), y)
    i_base = lut_idx(base, htable500['htable'])
    for k in (-10, -3, 7, 14):
        est = dti.TensorDirections.from_scheme(sc, fit_method=method, min_signal=1e-4 * 2.0 ** k)
        d = fit(est, y * y.dtype.type(2.0 ** k))
        assert est.last_unconverged() == 0
        assert np.array_equal(lut_idx(d, htable500['htable']), i_base), k
        if method == 'WLS':
            # a direct solve: each run is within the 1e-8 yardstick of the exact answer.  (NLLS stops where its cost, which is
            # flat to second order at the minimum, no longer moves in fp64: the parameters are defined to ~sqrt(1e-15) there,
            # so its axes are held to the LUT index here and to MINPACK in test_nlls_vs_minpack_synthetic.)
            assert axis_error(d, base).max() < 2e-8, k


def _raw_volume(htable500, seed=4):
    ht = htable500['htable']
    sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, htable500['dirs'])
    shape = (24, 20, 10)
    y, _ = S.noddi_signals(int(np.prod(shape)), K, ht, sch, seed=seed)
    img = np.asfortranarray((y.reshape(shape + (-1,)) * 1000.0).astype(np.float32))
    mask = (np.random.default_rng(2).uniform(size=shape) < 0.7).astype(np.uint8)
    return sch, K, ht, img, mask


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['WLS', 'NLLS'])
def test_evaluation_end_to_end(htable500, method):
    """raw volume -> maps with DTI_fit_method set: DIRs against the restatement; the maps are those of a fit that is handed
    the same directions as peaks"""
    import amico_amd
    sch, K, ht, img, mask = _raw_volume(htable500)
    sel = mask == 1

    def run(directions=None):
        ae = amico_amd.Evaluation()
        ae.set_config('DTI_fit_method', method)
        ae.set_data(img, sch, mask, directions=directions)
        ae.set_model('NODDI')
        ae.set_kernels(K, ht)
        ae.fit()
        return ae

    ae = run()
    y_ref, _ = signal_np.prepare_signal(img, mask, sch.b0_idx, sch.dwi_idx)
    assert np.array_equal(ae.y, y_ref)
    dirs = np.asarray(ae.DIRs, dtype=np.float64)
    if method == 'WLS':
        ref, ev = M.directions(y_ref, sch.b, sch.raw[:, :3], 'WLS', return_evals=True)
        _check_vs_ref(dirs, ref, ev, ht)
    else:
        est = type('E', (), {'last_unconverged': staticmethod(lambda: 0)})
        _nlls_check(est, y_ref, sch.b, sch.raw[:, :3], ht, dirs, 'end to end')
    assert ae.RESULTS['DIRs'].shape == img.shape[:3] + (3,) and not ae.RESULTS['MAPs'][~sel].any()
    assert np.array_equal(ae.RESULTS['DIRs'][sel], dirs.astype(np.float32))
    # the same image with those directions as peaks (float32, as a peaks file holds them)
    ae2 = run(directions=ae.RESULTS['DIRs'])
    same = lut_idx(dirs, ht) == lut_idx(ae.RESULTS['DIRs'][sel].astype(np.float64), ht)
    assert same.mean() > 0.999
    assert np.array_equal(ae.RESULTS['MAPs'][sel][same], ae2.RESULTS['MAPs'][sel][same])
    # and the method matters: the OLS axes are other axes
    ols = signal_np.dti_directions(y_ref, sch.b, sch.raw[:, :3])
    assert np.median(axis_error(dirs, ols)) > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['WLS', 'NLLS'])
def test_gather_with_directions_takes_the_two_kernel_route(method):
    """amx_prep_gather_directions_device_f32 with a WLS / NLLS handle = gather + amx_dti_directions_device_f32, bit for bit"""
    import torch
    from amico_amd import prep, dti, _capi
    sc = S.make_scheme()
    rng = np.random.default_rng(3)
    shape = (70, 9, 5)
    img = rng.uniform(50.0, 900.0, shape + (sc.nS,)).astype(np.float32)
    img[..., sc.b0_idx] += 600.0
    mask = (rng.uniform(size=shape) < 0.6).astype(np.uint8)
    sp = prep.SignalPreparation(sc, img, mask)
    td = dti.TensorDirections.from_scheme(sc, ctx=sp.ctx, fit_method=method)
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
    c.check(L.amx_prep_gather_directions_device_f32(c._h, sp._plan._h, td._dti._h, d_img.data_ptr(), norm, 0.0, y_b.data_ptr(),
                                                    mb_b.data_ptr(), d_b.data_ptr(), None))
    c.sync(None)
    assert torch.equal(y_a, y_b) and torch.equal(mb_a, mb_b)
    assert n > 1000 and torch.isfinite(d_a).all() and torch.equal(d_a, d_b)
    ols = dti.TensorDirections.from_scheme(sc, ctx=sp.ctx).fit(y_a.cpu().numpy().astype(np.float64))
    assert np.median(axis_error(d_a.cpu().numpy(), ols)) > 1e-4          # (not the fused OLS kernel's answer)
