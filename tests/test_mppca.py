"""The Marchenko-Pastur noise estimator (doEstimateNoise = 'MPPCA'; include/amico_amd.h "(f0++)"): what can be checked without a
device -- the eigenvalue algorithm the kernel uses as restated in tests/mppca_np.py, the estimator's bias on small synthetic volumes, the
launch arithmetic (amx_mppca_route) and the configuration rules of Evaluation.set_data.

The eigenvalue bound.  The restated algorithm (Householder tridiagonalisation, 56-step Sturm bisection) on the fp64 Gram matrix was compared
with numpy.linalg.eigvalsh of the Gram matrix accumulated in long double, on every eligible voxel of the inputs of CASES below (seeds
fixed): max |lambda - lambda_ref| = c eps (q + r) lambda_max with a worst c of 0.180 (w = 3, 17 volumes; 0.396 without the q term).  The
tests' constant is four times that: C_EIG = 0.72.  That measurement walked all voxels; the test below walks all voxels of the w = 3 cases
(where the worst c is) and a sample of two dozen of the w = 5 cases, whose matrices take longer."""
import os
import re

import numpy as np
import pytest

import mppca_np as M
from amico_amd import synthetic as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
EPS = np.finfo(np.float64).eps
C_MEASURED = 0.180
C_EIG = 4 * C_MEASURED
SIGMA = 5.0

# (spatial shape, volumes, patch edge): the shapes of tests/test_gpu_mppca.py
CASES = [((10, 10, 10), 15, 3), ((10, 10, 10), 16, 3), ((10, 10, 10), 17, 3), ((10, 10, 10), 20, 3), ((10, 10, 10), 27, 3),
         ((10, 10, 10), 32, 3), ((9, 9, 9), 40, 5), ((8, 8, 8), 130, 5), ((7, 7, 7), 512, 5)]


@pytest.mark.parametrize('shape,nS,w', CASES)
def test_eigenvalue_algorithm_against_long_double_gram(shape, nS, w):
    img, mask = M.synthetic(shape, nS, SIGMA, seed=nS + w)
    sel = mask == 1
    cs = np.argwhere(sel)
    if w == 5:
        cs = cs[:: max(1, len(cs) // 24)]             # w = 5: two dozen voxels spread over the mask, border and interior (w = 3: all)
    worst = 0.0
    for c in cs:
        X = M.patch_matrix(img, sel, c, w)
        if 2 * X.shape[1] < w ** 3:
            continue
        G, r, q = M.gram(X)
        ref = np.linalg.eigvalsh(M.gram(X, np.longdouble)[0].astype(np.float64))
        lam = M.eigvals_restated(G)
        assert np.all(np.diff(lam) >= 0)
        worst = max(worst, float(np.max(np.abs(lam - ref)) / (EPS * (q + r) * ref[-1])))
    print(f'{shape} x {nS}, w {w}: c = {worst:.3f} (bound {C_EIG})')
    assert 0 < worst <= C_EIG


def test_eigenvalue_algorithm_scales_exactly():
    """every threshold follows the matrix: the eigenvalues of 4^k G are 4^k times those of G, bit for bit"""
    img, mask = M.synthetic((6, 6, 6), 20, SIGMA, seed=3)
    X = M.patch_matrix(img, mask == 1, (3, 3, 3), 3)
    G = M.gram(X)[0]
    lam = M.eigvals_restated(G)
    for k in (-10, 14):
        assert np.array_equal(M.eigvals_restated(G * 4.0 ** k), lam * 4.0 ** k)


def test_eigenvalue_algorithm_degenerate_matrices():
    assert np.array_equal(M.eigvals_restated(np.zeros((5, 5))), np.zeros(5))
    lam = M.eigvals_restated(np.diag([3.0, 1.0, 2.0, 2.0]))
    assert np.allclose(lam, [1.0, 2.0, 2.0, 3.0], rtol=0, atol=4 * EPS * 3.0)
    v = np.arange(1.0, 7.0)
    lam = M.eigvals_restated(np.outer(v, v))          # rank one
    assert abs(lam[-1] - v @ v) <= 8 * EPS * (v @ v) and np.all(np.abs(lam[:-1]) <= 8 * EPS * (v @ v))


@pytest.mark.parametrize('shape,nS,w,lo,hi', [((10, 10, 10), 20, 3, 0.90, 1.02), ((10, 10, 10), 27, 3, 0.90, 1.02), ((10, 10, 10), 32, 3, 0.90, 1.02),
                                              ((9, 9, 9), 40, 5, 0.94, 1.02), ((8, 8, 8), 130, 5, 0.94, 1.02)])
def test_bias_bands(shape, nS, w, lo, hi):
    """four smooth components plus Gaussian noise: the median of sigma over the mask is a few percent low on small patches (the
    estimator's finite-size property), inside the band the issue quotes"""
    img, mask = M.synthetic(shape, nS, SIGMA, seed=nS + w)
    res = M.estimate(img, mask, [0], w)
    ratio = float(np.nanmedian(res['sigma']) / SIGMA)
    print(f'{shape} x {nS}, w {w}: median sigma / true = {ratio:.4f}, {int(np.isfinite(res["sigma"]).sum())} of {len(res["sigma"])} voxels eligible')
    assert lo <= ratio <= hi
    assert np.nanmax(res['signal']) <= 8              # four components and a little leakage, never the whole spectrum


def test_rule_on_a_flat_spectrum_and_on_zero():
    lam = np.full(10, 4.0 * 50)                       # pure noise of variance 4 at q = 50: everything is noise
    sigma, nsig, margin, pc = M.rule(lam, 50)
    assert sigma == 2.0 and nsig == 0 and pc == 9
    assert M.rule(np.zeros(6), 20)[3] == -1           # a zero patch: no p, not eligible


# ------------------------------------------------------------------ the launch arithmetic
def test_route_every_shape_fits_and_is_as_defined():
    from amico_amd import _capi
    for w in (3, 5):
        for nS in range(7, 513):
            for n in range((w ** 3 + 1) // 2, w ** 3 + 1):
                rt = _capi.mppca_route(nS, w, n, (w, w + 1, 40))
                assert rt['lds'] <= 160 * 1024, (nS, w, n)
                assert rt['r'] == min(nS, n) and rt['q'] == max(nS, n) and rt['gram'] == rt['r']
                assert rt['side'] == ('volumes' if nS <= n else 'patch')
                assert rt['eligible'] and rt['chunk'] % 4 == 0 and rt['chunk'] > 0
                assert rt['waves'] * rt['patches'] == 4 and rt['waves'] == (4 if w == 5 else 1)
    assert not _capi.mppca_route(40, 5, 62, (9, 9, 9))['eligible'] and _capi.mppca_route(40, 5, 63, (9, 9, 9))['eligible']
    assert _capi.mppca_route(512, 5, 125, (5, 5, 5))['lds'] == _capi.mppca_route(130, 5, 70, (8, 8, 8))['lds']   # sized for the launch


@pytest.mark.parametrize('nS,w,n,dims', [(40, 4, 30, (9, 9, 9)), (40, 7, 200, (9, 9, 9)), (513, 5, 100, (9, 9, 9)), (40, 5, 100, (9, 4, 9)),
                                         (40, 3, 20, (2, 9, 9)), (0, 3, 20, (9, 9, 9)), (40, 3, 28, (9, 9, 9))])
def test_route_refuses(nS, w, n, dims):
    from amico_amd import _capi
    with pytest.raises(ValueError):
        _capi.mppca_route(nS, w, n, dims)


# ------------------------------------------------------------------ configuration rules: all act in set_data, before anything is uploaded
class Reached(Exception):
    pass


def one_b0_image(shape=(6, 5, 7)):
    sch = S.make_scheme(1, ((1000.0, 8),), seed=1)
    return np.ones(shape + (sch.nS,), dtype=np.float32), sch


def stop_at_the_plan(monkeypatch):
    from amico_amd import prep

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(prep, 'SignalPreparation', stop)


@pytest.mark.parametrize('value', ['MPPCA', 'mppca', 'MpPca'])
def test_set_data_accepts_mppca_on_a_single_b0_scheme(value, monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image()
    ae = amico_amd.Evaluation()
    assert ae.get_config('noise_patch') == 5
    ae.set_config('doEstimateNoise', value)
    with pytest.raises(Reached):                      # every check passed: set_data went on to build the plan
        ae.set_data(img, sch)


@pytest.mark.parametrize('value', [True, 1, 'yes', 'PCA'])
def test_every_other_value_still_needs_b0_repeats(value, monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image()
    ae = amico_amd.Evaluation()
    ae.set_config('doEstimateNoise', value)
    with pytest.raises(RuntimeError, match='doEstimateNoise.*b0 repeats'):
        ae.set_data(img, sch)


@pytest.mark.parametrize('patch', [4, 7, 0, 5.0, '5', None, True])
def test_bad_noise_patch_is_a_value_error(patch, monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image()
    ae = amico_amd.Evaluation()
    ae.set_config('doEstimateNoise', 'MPPCA')
    ae.set_config('noise_patch', patch)
    with pytest.raises(ValueError, match='noise_patch'):
        ae.set_data(img, sch)


def test_noise_patch_is_not_read_without_mppca(monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image()
    ae = amico_amd.Evaluation()
    ae.set_config('noise_patch', 4)
    with pytest.raises(Reached):
        ae.set_data(img, sch)


@pytest.mark.parametrize('shape,patch,ok', [((6, 4, 7), 5, False), ((6, 4, 7), 3, True), ((2, 9, 9), 3, False), ((5, 5, 5), 5, True)])
def test_axis_shorter_than_the_patch_is_a_runtime_error(shape, patch, ok, monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image(shape)
    ae = amico_amd.Evaluation()
    ae.set_config('doEstimateNoise', 'MPPCA')
    ae.set_config('noise_patch', patch)
    with pytest.raises(Reached if ok else RuntimeError, match=None if ok else 'doEstimateNoise.*noise_patch'):
        ae.set_data(img, sch)


def test_debias_keeps_its_own_b0_check(monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    sch = S.make_scheme(0, ((1000.0, 8),), seed=1)
    img = np.ones((6, 6, 6, sch.nS), dtype=np.float32)
    ae = amico_amd.Evaluation()
    ae.set_config('doEstimateNoise', 'MPPCA')
    with pytest.raises(Reached):                      # no b0 volume at all: the estimator itself does not mind
        ae.set_data(img, sch)
    ae.set_config('doDebiasSignal', True)
    with pytest.raises(RuntimeError, match='No b0 volume'):
        ae.set_data(img, sch)


def test_bindings_are_declared():
    from amico_amd import _capi, noise
    hdr = open(os.path.join(ROOT, 'include', 'amico_amd.h')).read()
    declared = set(re.findall(r'\b(amx_[a-z0-9_]+)\s*\(', hdr))
    L = _capi.lib()
    for n in ['amx_prep_noise_mppca_device', 'amx_mppca_route']:
        assert n in declared and n in _capi.SYMBOLS and getattr(L, n).argtypes is not None, n
    assert 'clamp(c_a - h, 0, D_a - w)' in hdr and '4 sqrt(gamma_p)' in hdr
    assert callable(_capi.Prep.noise_mppca_device) and callable(_capi.mppca_route)
    assert callable(noise.estimate_mppca_device) and callable(noise.estimate_mppca)
    assert noise.is_mppca('mppca') and not noise.is_mppca(True) and not noise.is_mppca('PCA')
