"""The Marchenko-Pastur denoiser (doDenoise = 'MPPCA'; include/amico_amd.h "(f0+++)"): what can be checked without a device -- the
kernel's algorithm as restated in tests/mppca_denoise_np.py against the float64 SVD reference, the reference itself, the launch arithmetic
(amx_mppca_denoise_route) and the configuration rules of Evaluation.set_data.

The bound.  A denoised row may differ from the reference's by

    |x^ - x^_ref|_2  <=  C_DEN eps (q + r) (lambda_max / gap) |x_c|_2,      gap = lambda_ref[cut] - lambda_ref[cut - 1]

(Davis-Kahan on a Gram matrix whose rounding is what C_EIG of tests/test_mppca.py measures).  The restated algorithm was compared with the
reference on every eligible voxel of every input of tests/test_gpu_mppca_denoise.py (seeds fixed; n_signal agreed on all of them): the
worst constant was 2.772 (w = 3, 17 volumes, n_signal = 1, where lambda_max / gap is about 1: a relative row error of 2.3e-14, a hundred
eps after r reflectors each way); 2.64 on (3, 6, 5) x 20, 2.2 to 2.3 at 15, 16 and 20 volumes, 1.07 at 32, 0.50 at 27, 0.42 at w = 5 with 40
volumes and under 1e-3 on every other w = 5 input and on the images of high rank, whose lambda_max / gap is 1e4 to 3e11 (relative row
errors up to 1.5e-10 at sigma = 1e-3 on amplitude 100).  The tests' constant is four times the worst: C_DEN = 11.09.  That measurement
walked all voxels; the test below walks a sample of every input."""
import os
import re

import numpy as np
import pytest

import mppca_denoise_np as D
import mppca_np as M
from test_mppca import SIGMA, one_b0_image, stop_at_the_plan, Reached

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
C_MEASURED = 2.772
C_DEN = 4 * C_MEASURED

# (spatial shape, volumes, patch edge, every how-manieth voxel): the shapes of tests/test_gpu_mppca_denoise.py
CASES = [((10, 10, 10), 15, 3, 8), ((10, 10, 10), 16, 3, 8), ((10, 10, 10), 17, 3, 4), ((10, 10, 10), 20, 3, 8), ((10, 10, 10), 27, 3, 8),
         ((10, 10, 10), 32, 3, 8), ((9, 9, 9), 40, 5, 16), ((8, 8, 8), 130, 5, 64), ((7, 7, 7), 512, 5, 64)]
HIGHRANK = [((6, 6, 6), 20, 12, 1.0, 3, 8), ((7, 7, 7), 60, 40, 0.3, 5, 24), ((7, 7, 7), 60, 8, 1e-3, 5, 24)]


def worst_constant(img, mask, w, step):
    sel = mask == 1
    cs = np.argwhere(sel)
    worst, count = 0.0, 0
    for v in range(0, len(cs), step):
        X = M.patch_matrix(img, sel, cs[v], w)
        if 2 * X.shape[1] < w ** 3:
            continue
        col = D.centre_column(sel, cs[v], w)
        G, r, q = M.gram(X)
        lam = np.sort(np.linalg.eigvalsh(G))
        _, nsig, _, pc = M.rule(lam, q)
        x, s = D.restated_row(X, col)
        assert pc >= 0 and s == int(nsig) > 0
        ref = D.truncated_column(X, s, col)
        cut = r - s
        b = D.EPS * (q + r) * lam[-1] / (lam[cut] - lam[cut - 1]) * np.linalg.norm(X[:, col])
        worst = max(worst, float(np.linalg.norm(x - ref) / b))
        count += 1
    return worst, count


@pytest.mark.parametrize('shape,nS,w,step', CASES)
def test_restated_algorithm_against_the_svd(shape, nS, w, step):
    img, mask = M.synthetic(shape, nS, SIGMA, seed=nS + w)
    worst, count = worst_constant(img, mask, w, step)
    print(f'{shape} x {nS}, w {w}: {count} voxels, c = {worst:.3g} (bound {C_DEN})')
    assert count >= 4 and 0 < worst <= C_DEN


@pytest.mark.parametrize('shape,nS,K,sigma,w,step', HIGHRANK)
def test_restated_algorithm_on_images_of_high_rank(shape, nS, K, sigma, w, step):
    """the signal set (s of up to 8 of 20), the complement (s of 37 to 40 of 60), and lambda_max / gap of 3e11"""
    img, _, mask = D.highrank(shape, nS, K, sigma, seed=1)
    worst, count = worst_constant(img, mask, w, step)
    print(f'{shape} x {nS}, K {K}, sigma {sigma}: {count} voxels, c = {worst:.3g} (bound {C_DEN})')
    assert count >= 8 and 0 < worst <= C_DEN


def test_twisted_vectors_on_degenerate_tridiagonals():
    """a split matrix (a zero off-diagonal) and a diagonal one: finite, orthonormal after Gram-Schmidt, and eigenvectors"""
    d = np.array([4.0, 1.0, 3.0, 2.0, 5.0])
    for e in (np.array([1.0, 0.0, 0.5, 0.25]), np.zeros(4)):
        T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        lam = M.bisect(d, e)
        U = D.orthonormalise(D.twisted_vectors(d, e, lam[3:]))
        assert np.isfinite(U).all() and np.allclose(U.T @ U, np.eye(2), atol=1e-14)
        assert np.allclose(T @ U, U * lam[3:], atol=1e-13)


def test_reference_reproduces_a_noise_free_image_of_rank_k():
    """small integers: the float32 image has rank 4 exactly and the SVD truncated at 4 gives it back to rounding (the rule itself finds no p
    among eigenvalues that are rounding alone: such a voxel is not eligible); with a little noise the rule says 4 and the row is the clean
    one to a few sigma"""
    rng = np.random.default_rng(3)
    shape, nS, K, w = (6, 6, 6), 20, 4, 3
    prof = rng.integers(1, 16, size=(K, nS)).astype(np.float64)
    wts = rng.integers(0, 8, size=shape + (K,)).astype(np.float64)
    clean = wts @ prof
    img = clean.astype(np.float32)
    assert np.array_equal(img, clean)
    sel = np.ones(shape, dtype=bool)
    for c in np.argwhere(sel)[::7]:
        X = M.patch_matrix(img, sel, c, w)
        col = D.centre_column(sel, c, w)
        assert np.linalg.matrix_rank(X) == K
        assert np.max(np.abs(D.truncated_column(X, K, col) - X[:, col])) <= 64 * D.EPS * np.abs(X).max()
    sigma = 1e-3
    noisy = (clean + sigma * rng.standard_normal(clean.shape)).astype(np.float32)
    ref = D.reference(noisy, sel.astype(np.uint8), w)
    assert (ref['status'] == 0).all() and (ref['signal'] == K).all()
    assert np.max(np.abs(ref['rows'] - clean.reshape(-1, nS))) < 5 * sigma


def test_denoising_brings_a_noisy_image_nearer_the_clean_one():
    """a sanity test, not an accuracy bound"""
    shape, nS, w = (9, 9, 9), 40, 5
    img, mask = M.synthetic(shape, nS, SIGMA, seed=nS + w)
    clean, _ = M.synthetic(shape, nS, 0.0, seed=nS + w)
    ref = D.reference(img, mask, w)
    ok = ref['status'] == 0
    noisy, clean = img[mask == 1][ok].astype(np.float64), clean[mask == 1][ok].astype(np.float64)
    e_noisy, e_den = np.sqrt(np.mean((noisy - clean) ** 2)), np.sqrt(np.mean((ref['rows'][ok] - clean) ** 2))
    print(f'rms error against the clean image: noisy {e_noisy:.3f}, denoised {e_den:.3f}')
    assert 0.9 * SIGMA < e_noisy < 1.1 * SIGMA and e_den < 0.6 * e_noisy


# ------------------------------------------------------------------ the launch arithmetic
def test_route_every_shape_fits_and_no_route_has_a_cap():
    from amico_amd import _capi
    for w in (3, 5):
        for nS in range(1, 513):
            for n in range(0, w ** 3 + 1):
                dims = (w, w + 1, 40)
                rt, base = _capi.mppca_denoise_route(nS, w, n, dims), _capi.mppca_route(nS, w, n, dims)
                assert base['lds'] < rt['lds'] <= 160 * 1024 and rt['lds'] == rt['per_patch'] * rt['patches'], (nS, w, n)
                assert rt['cap'] == 0 and rt['capacity'] >= rt['r'] // 2
                for k in ('r', 'q', 'side', 'waves', 'patches', 'eligible'):
                    assert rt[k] == base[k]
    # k_mppca's own launch has not moved: the figures of DESIGN 7n
    assert _capi.mppca_route(512, 5, 125, (5, 5, 5))['lds'] == 150128 and _capi.mppca_route(20, 3, 27, (9, 9, 9))['lds'] == 4 * 9656
    with pytest.raises(ValueError):
        _capi.mppca_denoise_route(513, 5, 100, (9, 9, 9))
    with pytest.raises(ValueError):
        _capi.mppca_denoise_route(40, 5, 100, (9, 4, 9))


# ------------------------------------------------------------------ configuration rules: all act in set_data, before anything is uploaded
@pytest.mark.parametrize('value', ['MPPCA', 'mppca', True])
def test_set_data_accepts_the_key(value, monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image()
    ae = amico_amd.Evaluation()
    assert ae.get_config('doDenoise') is False and ae.get_config('doSaveDenoisedDWI') is False
    ae.set_config('doDenoise', value)
    ae.set_config('doDebiasSignal', True)             # no DWI-SNR given: the launch delivers the estimate
    with pytest.raises(Reached):
        ae.set_data(img, sch)


@pytest.mark.parametrize('value', ['PCA', 'yes', 1, 5.0])
def test_any_other_value_is_a_value_error(value, monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    img, sch = one_b0_image()
    ae = amico_amd.Evaluation()
    ae.set_config('doDenoise', value)
    with pytest.raises(ValueError, match='doDenoise'):
        ae.set_data(img, sch)


def test_patch_rules_are_the_estimator_s(monkeypatch):
    import amico_amd
    stop_at_the_plan(monkeypatch)
    ae = amico_amd.Evaluation()
    ae.set_config('doDenoise', True)
    img, sch = one_b0_image((6, 4, 7))
    with pytest.raises(RuntimeError, match='noise_patch'):
        ae.set_data(img, sch)
    ae.set_config('noise_patch', 3)
    with pytest.raises(Reached):
        ae.set_data(img, sch)
    ae.set_config('noise_patch', 4)
    with pytest.raises(ValueError, match='noise_patch'):
        ae.set_data(img, sch)
    ae.set_config('noise_patch', 3)
    ae.set_config('doEstimateNoise', True)            # the b0 estimator keeps its own rule beside the denoiser
    with pytest.raises(RuntimeError, match='doEstimateNoise.*b0 repeats'):
        ae.set_data(img, sch)


def test_bindings_are_declared():
    from amico_amd import _capi, noise
    hdr = open(os.path.join(ROOT, 'include', 'amico_amd.h')).read()
    declared = set(re.findall(r'\b(amx_[a-z0-9_]+)\s*\(', hdr))
    L = _capi.lib()
    for n in ['amx_prep_noise_mppca_denoise_device', 'amx_mppca_denoise_route']:
        assert n in declared and n in _capi.SYMBOLS and getattr(L, n).argtypes is not None, n
    assert callable(_capi.Prep.noise_mppca_denoise_device) and callable(_capi.mppca_denoise_route)
    assert callable(noise.denoise_mppca_device) and callable(noise.denoise_mppca)
    assert noise.is_denoise('mppca') and noise.is_denoise(True) and not noise.is_denoise(False) and not noise.is_denoise(None)
