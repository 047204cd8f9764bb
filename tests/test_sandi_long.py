"""The yardstick the GPU tests of the long-protocol SANDI route lean on (tests/test_gpu_sandi_long.py), pinned on the CPU:

  * the oracle's coefficients on un-averaged schemes of 129, 306 and 512 volumes are the optimum of the Gram-space problem the
    GPU route solves -- H = A'A + lambda2 I, c = A'y: g = c - H x vanishes on the support and is <= 0 off it -- and equal an
    independent solver's (scipy nnls on the augmented system [A; sqrt(lambda2) I]);
  * the residual the error maps need follows from c, y'y and G = A'A alone: rss = y'y - 2 x'c + x'G x, with the RESCALED x
    (models.pyx:1571 then 1615).  That quirk keeps rmse at ~0.4 on unit signals, so the identity does not cancel.
"""
import numpy as np
import pytest

LAM2 = 5e-3
SCHEMES = {129: dict(ndir_per_shell=25, n_b0=4), 306: {}, 512: dict(ndir_per_shell=100, n_b0=12)}


@pytest.fixture(scope='module', params=sorted(SCHEMES))
def case(request):
    from amico_amd import synthetic as S
    from oracle import oracle
    sch = S.make_sandi_scheme(**SCHEMES[request.param])
    assert sch.nS == request.param
    K, Rs, d_in, d_isos = S.sandi_kernels(sch)
    y = S.sandi_signals(100, K, sch, seed=3, navg=1)
    ref = oracle.sandi_fit(y, K, Rs, d_in, d_isos, 0.0, LAM2, rmse=True, nrmse=True, return_x=True)
    A = np.asarray(K['signal'], dtype=np.float64)
    return dict(A=A, y=y, norms=K['norms'], ref=ref, x=ref['x'] / K['norms'][None, :])


def test_oracle_is_the_gram_space_optimum(case):
    A, y, x = case['A'], case['y'], case['x']
    H = A.T @ A + LAM2 * np.eye(A.shape[1])
    g = y @ A - x @ H
    assert x.min() >= 0.0
    assert np.abs(g[x > 0]).max() < 1e-10
    assert g[x == 0].max() < 1e-10


def test_oracle_matches_nnls_on_the_augmented_system(case):
    from scipy.optimize import nnls
    A, y, x = case['A'], case['y'], case['x']
    n = A.shape[1]
    aug = np.vstack([A, np.sqrt(LAM2) * np.eye(n)])
    xn = np.stack([nnls(aug, np.concatenate([yi, np.zeros(n)]), maxiter=10000)[0] for yi in y])
    assert np.abs(xn - x).max() < 1e-9


def test_gram_identity_gives_the_residual(case):
    A, y, ref = case['A'], case['y'], case['ref']
    xt = ref['x']                                              # rescaled, as the reference takes the residual
    c = y @ A
    rss_true = ((y - xt @ A.T) ** 2).sum(axis=1)
    rss_gram = (y * y).sum(axis=1) - 2.0 * (xt * c).sum(axis=1) + np.einsum('ij,jk,ik->i', xt, A.T @ A, xt)
    assert np.abs(rss_gram - rss_true).max() < 1e-12 * max(1.0, rss_true.max())
    nS = A.shape[0]
    assert np.abs(np.sqrt(np.maximum(rss_gram, 0.0) / nS) - ref['rmse']).max() < 1e-12
    assert ref['rmse'].mean() > 0.1                            # the quirk: nothing near zero to cancel
