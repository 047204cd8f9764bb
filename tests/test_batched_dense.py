"""The algorithm of k_batched_big restated in numpy (batched_dense_np.py) on every input of tests/test_gpu_batched_dense.py, against
scipy's NNLS and the oracle's LARS: that the method converges -- thresholds, rank guard and refinement included -- is shown here, on
the CPU; the GPU tests then hold the kernel to the same numbers.  And the binding of the two new entry points."""
import inspect
import os
import re

import numpy as np
import pytest

import batched_dense_np as B


@pytest.mark.parametrize('m,n', list(B.SUPPORT_CASES))
def test_model_finds_the_prescribed_supports(m, n):
    from scipy.optimize import nnls as scipy_nnls
    A, y, xt, sizes = B.support_case(m, n)
    G = A.T @ A
    rows = range(len(y)) if n <= 64 else range(0, len(y), B.VOXELS_PER_SIZE)      # (the large shapes: one voxel of every size)
    for v in rows:
        xs, rs = scipy_nnls(A, y[v], maxiter=50 * n)
        # the construction: scipy finds the prescribed support and x_true itself; off the support the dual values keep a strict margin
        # (-0.009 .. -0.03 on these shapes: nine orders above the solver's thresholds)
        assert (xs > 0).sum() == sizes[v] and np.abs(xs - xt[v]).max() < 1e-12
        w = A.T @ (y[v] - A @ xt[v])
        assert w[xt[v] == 0].max() < -5e-3
        x, rn, info = B.solve(A, y[v], G=G)
        assert info['status'] == 'ok' and info['dropped'] == 0, info
        assert np.array_equal(x > 0, xt[v] > 0)
        assert np.abs(x - xt[v]).max() < 1e-9 and abs(rn - rs) < 1e-9
        gp, gz = B.kuhn_tucker(A, y[v], x)
        assert gp < 1e-9 and gz < 1e-9
        # lasso at (1e-4, 1e-4): the same support sizes
        xl, _, info = B.solve(A, y[v], 1e-4, 1e-4, G=G)
        assert info['status'] == 'ok' and (xl > 0).sum() == sizes[v]


@pytest.mark.parametrize('lam1,lam2', B.ELASTIC_NET_LAMBDAS)
def test_model_matches_the_oracle_on_nearly_collinear_atoms(htable500, lam1, lam2):
    from oracle import oracle
    A2, y, idx = B.elastic_net_case(htable500)
    G = np.einsum('dmi,dmj->dij', A2, A2)
    sizes = []
    for v in range(0, len(y), 5):
        A = A2[idx[v]]
        x, _, info = B.solve(A, y[v], lam1, lam2, G=G[idx[v]])
        xo = oracle.lasso(A, y[v], lam1, lam2)[0]
        assert info['status'] == 'ok', info
        assert np.array_equal(x > 0, xo > 0) and np.abs(x - xo).max() < 1e-9
        gp, gz = B.kuhn_tucker(A, y[v], x, lam1, lam2)
        assert gp < 1e-9 and gz < 1e-9
        sizes.append(int((x > 0).sum()))
    if lam1 == 0.0:                                                     # both kinds of voxel: beyond the 48-atom pass and inside the main pass
        assert max(sizes) > 48 and min(sizes) <= 16, (min(sizes), max(sizes))


def test_model_settles_a_wide_dictionary_without_a_ridge():
    """60 x 100, lambda2 = 0: H_PP is singular once a block step gathers more than 60 atoms -- the rank guard, then single exchanges"""
    from scipy.optimize import nnls as scipy_nnls
    A, y = B.wide_case()
    guarded = 0
    for v in range(len(y)):
        xs, rs = scipy_nnls(A, y[v], maxiter=5000)
        assert (xs > 0).sum() == 60 and rs < 1e-12 and np.linalg.cond(A[:, xs > 0]) <= 600
        x, rn, info = B.solve(A, y[v])
        assert info['status'] == 'ok' and info['steps'] <= 4 * 100 + 16, info
        guarded += info['dropped'] > 0
        assert x.min() >= 0.0 and (x > 0).sum() <= 60
        assert np.abs(A @ x - A @ xs).max() < 1e-8
        gp, gz = B.kuhn_tucker(A, y[v], x)
        bound = 1e-9 * max(1.0, np.linalg.norm(y[v]))
        assert gp < bound and gz < bound
    assert guarded > 0                                                  # the case does reach the rank guard


def test_model_is_scale_equivariant(htable500):
    A, y, xt, sizes = B.support_case(200, 60)
    G = A.T @ A
    A2, y2, idx = B.elastic_net_case(htable500, 40)
    for c in B.SCALES:
        for v in range(0, len(y), 3):
            x1 = B.solve(A, y[v], G=G)[0]
            xc = B.solve(A, c * y[v], G=G)[0]
            assert np.array_equal(x1 > 0, xc > 0) and np.abs(xc / c - x1).max() < 1e-9
        for v in range(0, 40, 4):
            x1 = B.solve(A2[idx[v]], y2[v], 2e-4, 1e-3)[0]
            xc = B.solve(A2[idx[v]], c * y2[v], 2e-4 * c, 1e-3)[0]
            assert np.array_equal(x1 > 0, xc > 0) and np.abs(xc / c - x1).max() < 1e-9


def test_model_reports_what_it_cannot_settle():
    """an all-zero signal is x = 0 at once; a step cap of nothing is 'itcap', never a result passed off as good"""
    A, y, _, _ = B.support_case(120, 56)
    x, rn, info = B.solve(A, np.zeros(120))
    assert not x.any() and rn == 0.0 and info['status'] == 'ok'
    x, rn, info = B.solve(A, y[-1], max_steps=0)
    assert info['status'] == 'itcap' and x.min() >= 0.0 and abs(rn - np.linalg.norm(y[-1] - A @ x)) < 1e-12


def test_binding_of_the_dense_entry_points():
    from amico_amd import _capi
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, '..', 'include', 'amico_amd.h')) as fh:
        header = fh.read()
    for name in ('amx_dict_set_dense', 'amx_batched_last_dense'):
        assert name in _capi.SYMBOLS
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
    sig = inspect.signature(_capi.Dict.__init__)
    assert 'dense' in sig.parameters and sig.parameters['dense'].default is False
    assert callable(_capi.Dict.set_dense) and callable(_capi.Context.last_dense)
