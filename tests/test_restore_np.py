"""The restatement of the robust tensor fit (tests/restore_np.py) pinned on rows whose answer is known, the scenes the GPU tests
(tests/test_gpu_dti_restore.py) share with it, and the host-side argument rules of the robust fit.  No GPU.
"""
import numpy as np
import pytest

import amico_amd.synthetic as S
import dti_methods_np as M
import restore_np as R

SIGMA = 1.0 / 30.0              # the noise level of the noisy scene: noddi_signals at SNR 30, divided by the b0 mean
PLANTED_SIGMA = 0.02            # noise-free rows: any sigma well below the planted +0.5 and above rounding


def scheme(n_vol):
    """the schemes of the robust tests by volume count (8: the shortest that leaves an outlier to find; 33 = 3 b0 + 30, no multiple
    of the kernel's 8 lanes per voxel; 99: the standard protocol; 130, 288, 512: shorter and shorter LDS tiles)"""
    if n_vol == 99:
        return S.make_scheme()
    n_b0 = {8: 1, 33: 3, 130: 10, 288: 8, 512: 12}[n_vol]
    n = n_vol - n_b0
    shells = ((1000.0, n),) if n_vol <= 33 else ((700.0, n // 3), (1500.0, n // 3), (2500.0, n - 2 * (n // 3)))
    return S.make_scheme(n_b0=n_b0, shells=shells, seed=n_vol)


def planted_rows(sc, n, seed=0, every=1, amp=0.5):
    """noise-free single-tensor rows S = exp(-b g'Dg), D = Q diag(l) Q' with l1 > l2 > l3 (the closed-form rows of the DTI tests),
    and +amp on nS // 12 (at least one) random volumes of every `every`-th voxel -> (y [n, nS], axis [n, 3], evals [n, 3], planted bool [n, nS])"""
    rng = np.random.default_rng(seed)
    b, g = sc.b, sc.raw[:, :3]
    y, axis, evals = np.empty((n, sc.nS)), np.empty((n, 3)), np.empty((n, 3))
    planted = np.zeros((n, sc.nS), dtype=bool)
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        l = np.array([1.7e-3, 0.5e-3, 0.3e-3]) * rng.uniform(0.7, 1.1)
        D = (q * l) @ q.T
        y[i] = np.exp(-b * np.einsum('ij,jk,ik->i', g, D, g))
        axis[i], evals[i] = q[:, 0], l
        if i % every == 0:
            planted[i, rng.choice(sc.nS, max(sc.nS // 12, 1), replace=False)] = True
    y[planted] += amp
    return y, axis, evals, planted


_NOISY = {}


def noisy_rows(htable500, n=300, n_vol=99, seed=21):
    """noddi_signals at SNR 30 with +0.6 on 0 .. 7 random volumes of each voxel -> (scheme, y [n, nS]); made once per shape"""
    key = (n, n_vol, seed)
    if key not in _NOISY:
        sc = scheme(n_vol)
        K = S.noddi_kernels(sc, htable500['dirs'])
        y, _ = S.noddi_signals(n, K, htable500['htable'], sc, seed=seed, snr=30.0)
        rng = np.random.default_rng(seed + 1)
        for i in range(n):
            y[i, rng.choice(sc.nS, rng.integers(0, 8), replace=False)] += 0.6
        y = y.astype(np.float32).astype(np.float64)                      # (float32 values, as every prepared signal is)
        y.setflags(write=False)
        _NOISY[key] = (sc, y)
    return _NOISY[key]


def one_minus_cos(a, b):
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    return 1.0 - np.abs((a * b).sum(1))


@pytest.mark.parametrize('n_vol', [33, 99])
def test_planted_outliers_are_found(n_vol):
    sc = scheme(n_vol)
    y, axis, evals, planted = planted_rows(sc, 24, seed=n_vol)
    X = M.design(sc.b, sc.raw[:, :3])
    got = R.restore(y, X, PLANTED_SIGMA)
    assert got['entered'].all() and got['refitted'].all() and not got['capped'].any() and not got['few'].any()
    assert np.array_equal(got['mask'], planted)
    assert np.array_equal(got['outliers'], planted.sum(1))
    dirs, ev = M.decompose(got['params'])
    err = one_minus_cos(dirs, axis)
    plain = one_minus_cos(M.decompose(M.nlls_params(y, X, tight=True))[0], axis)
    print('%d volumes: 1 - |cos| robust max %.3g, plain NLLS median %.3g (%.1f degrees), trips max %d'
          % (n_vol, err.max(), np.median(plain), np.degrees(np.arccos(1.0 - np.median(plain))), got['trips'].max()))
    assert err.max() < 1e-10
    assert np.median(plain) > 1e-3                                   # the plain fit is off by degrees: the outliers matter
    assert (np.abs(ev - evals) / evals[:, :1]).max() < 1e-9
    # dipy's own route finds every planted outlier on the same rows (it may call further samples outliers: it stops earlier)
    _, mask = R.restore_dipy_route(y, X, PLANTED_SIGMA)
    assert (mask & planted).sum() == planted.sum()


def test_routes_agree_on_the_gpu_scene(htable500):
    """one trial per reweighting (the kernel's route) against every reweighted problem solved to its minimum: equal verdicts"""
    sc, y = noisy_rows(htable500)
    X = M.design(sc.b, sc.raw[:, :3])
    y = y[:60]
    a = R.restore(y, X, SIGMA, route='trial')
    b = R.restore(y, X, SIGMA, route='converged')
    sure = (a['margin'] > 1e-4) & (b['margin'] > 1e-4) & ~a['capped'] & ~b['capped']
    print('entered %d of %d, trips median %d max %d, verdicts compared on %d'
          % (a['entered'].sum(), len(y), np.median(a['trips'][a['entered']]), a['trips'].max(), sure.sum()))
    assert a['entered'].sum() >= 40 and sure.mean() >= 0.99
    assert np.array_equal(a['mask'][sure], b['mask'][sure])
    r_a = M._data(y, X, None) - np.exp(a['params'] @ X.T)
    r_b = M._data(y, X, None) - np.exp(b['params'] @ X.T)
    assert np.abs(r_a - r_b)[sure].max() < 1e-6


def test_cap_is_a_path_at_8_volumes():
    """with 8 volumes a share of the voxels cycles in step 3 until the cap: they keep their last accepted iterate and are counted"""
    sc = scheme(8)
    rng = np.random.default_rng(5)
    y, _, _, _ = planted_rows(sc, 60, seed=8, amp=1.5)
    y = np.abs(y + rng.normal(scale=SIGMA, size=y.shape))
    got = R.restore(y, M.design(sc.b, sc.raw[:, :3]), SIGMA)
    print('8 volumes: entered %d, refitted %d, capped %d, fewer than 7 inliers %d' % tuple(got[k].sum() for k in ('entered', 'refitted', 'capped', 'few')))
    assert got['capped'].any() and got['trips'].max() == R.TRIP_CAP
    assert np.isfinite(got['params']).all()
    assert (got['outliers'][got['refitted']] <= sc.nS - 7).all()
    assert not (got['capped'] & ~got['entered']).any()


def test_sigma_rules():
    """host-side: checked before a context or a device is needed"""
    from amico_amd import dti, _capi
    b = np.array([0.0] + [1000.0] * 7)
    g = np.vstack([np.zeros(3), np.eye(3), np.array([[1, 1, 0], [1, 0, 1], [0, 1, 1], [1, -1, 0]]) / np.sqrt(2)])
    for name in dti.ROBUST_METHODS:
        with pytest.raises(NotImplementedError, match='sigma'):
            dti.TensorDirections(b, g, fit_method=name, sigma=None)
        for bad in (0.0, -1.0, float('nan'), float('inf'), 'x', [0.1, 0.2], True):
            with pytest.raises(ValueError, match='sigma'):
                dti.TensorDirections(b, g, fit_method=name, sigma=bad)
    with pytest.raises(ValueError, match='sigma belongs to the robust'):
        dti.TensorDirections(b, g, fit_method='NLLS', sigma=0.1)
    w, x = np.zeros((7, 8)), np.zeros((8, 7))
    with pytest.raises(ValueError, match='sigma'):
        _capi.Dti(None, w, design=x, method='RESTORE')
    with pytest.raises(ValueError, match='sigma'):
        _capi.Dti(None, w, design=x, method='RESTORE', sigma=-2.0)
    with pytest.raises(ValueError, match='sigma belongs'):
        _capi.Dti(None, w, design=x, method='WLS', sigma=0.1)
    assert _capi.Dti.METHODS['RESTORE'] == 3
    assert dti.FIT_METHODS == {'OLS': 'OLS', 'LS': 'OLS', 'WLS': 'WLS', 'NLLS': 'NLLS'}


def test_sigma_resolution():
    from amico_amd import dti
    for name in dti.ROBUST_METHODS:
        assert dti.resolve_sigma(name, 0.05, 30.0, True) == 0.05                     # DTI_sigma wins
        assert dti.resolve_sigma(name, None, 30.0, True) == 1.0 / 30.0               # 1 / DWI-SNR on normalised signals
        assert dti.resolve_sigma(name, None, 30.0, False) is None                    # not normalised: no unit to turn the SNR into
        assert dti.resolve_sigma(name, None, None, True) is None
        for bad in (0.0, -0.1, float('nan'), float('inf'), 'a'):
            with pytest.raises(ValueError, match='sigma'):
                dti.resolve_sigma(name, bad, 30.0, True)
        for bad in (0.0, -3.0, float('nan'), float('inf'), 'a'):
            with pytest.raises(ValueError, match='DWI-SNR'):
                dti.resolve_sigma(name, None, bad, True)
    assert dti.resolve_sigma('NLLS', 0.05, 30.0, True) is None
    with pytest.raises(ValueError, match='DTI fit method must be one of'):
        dti.resolve_sigma('GLS', 0.05)


def test_evaluation_rejects_bad_sigma_before_upload():
    import amico_amd
    sc = S.make_scheme()
    for key, bad in (('DTI_sigma', -1.0), ('DTI_sigma', float('nan')), ('DWI-SNR', 0.0)):
        ae = amico_amd.Evaluation()
        assert ae.get_config('DTI_sigma') is None
        ae.niiDWI_img = np.zeros((2, 2, 2, sc.nS), dtype=np.float32)
        ae.scheme = sc
        ae.model = type('M', (), {'id': 'NODDI', 'name': 'NODDI'})()
        ae.KERNELS = {'model': 'NODDI'}
        ae.set_config('DTI_fit_method', 'RESTORE')
        ae.set_config(key, bad)
        with pytest.raises(ValueError, match='sigma|DWI-SNR'):
            ae.fit()
