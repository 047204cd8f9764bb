"""amx_nnls_batched / amx_lasso_batched on a dictionary marked dense (amx_dict_set_dense, Dict(ctx, A, dense=True)): no voxel is refused for
the size of its support -- what the 48-atom re-run pass cannot hold goes to k_batched_big (csrc/amx_batched_big.hip).  The inputs are those of
batched_dense_np.py, on which tests/test_batched_dense.py holds the numpy restatement of the kernel to the same bounds on the CPU.
Every test makes a context of its own: amx_last_path of the batched calls names every launch since the context's last model fit."""
import functools

import numpy as np
import pytest

import batched_dense_np as B

pytestmark = pytest.mark.gpu


def _support_problem(m, n, sizes, rng):
    """dictionary [m, n] with m > n and signals whose NNLS optimum is a given support P of k atoms: y = A_P x_P + r, x_P in
    [0.5, 1.5], with a residual r (2 % of the signal: a little noise the optimum cannot absorb) orthogonal to the support's columns
    and with A_j' r equal and negative for every other atom -- then x_P is the NNLS solution itself, with a strict margin
    (the construction of tests/test_gpu_amplitude.py; a support of k = n atoms cannot be made this way: the largest is n - 1)"""
    A = np.abs(rng.normal(size=(m, n))) + 0.2
    A /= np.linalg.norm(A, axis=0, keepdims=True)
    ys, xs = [], []
    for k in sizes:
        P = np.sort(rng.choice(n, k, replace=False))
        Z = np.setdiff1d(np.arange(n), P)
        x = np.zeros(n)
        x[P] = rng.uniform(0.5, 1.5, k)
        Q, _ = np.linalg.qr(A[:, P])
        B_ = A[:, Z] - Q @ (Q.T @ A[:, Z])                            # the other atoms off the support's span
        r = -B_ @ np.linalg.solve(B_.T @ B_, np.ones(len(Z)))          # A_Z' r = -1, A_P' r = 0
        y = A @ x + 0.02 * np.linalg.norm(A @ x) * r / np.linalg.norm(r)
        ys.append(y)
        xs.append(x)
    return A, np.array(ys), np.array(xs)


@functools.lru_cache(maxsize=None)
def _support_case(m, n):
    """(A, y, x_true, sizes, scipy's rnorm) of one shape: made once, shared by the tests, never written to"""
    from scipy.optimize import nnls as scipy_nnls
    sizes = np.repeat(np.array(B.SUPPORT_CASES[(m, n)]), B.VOXELS_PER_SIZE)
    A, y, xt = _support_problem(m, n, sizes, np.random.default_rng(m * n))
    A0, y0, xt0, _ = B.support_case(m, n)
    assert np.array_equal(A, A0) and np.array_equal(y, y0) and np.array_equal(xt, xt0)      # the numbers the CPU tests ran on
    rn = np.array([scipy_nnls(A, yy, maxiter=50 * n)[1] for yy in y])
    for a in (A, y, xt, sizes, rn):
        a.setflags(write=False)
    return A, y, xt, sizes, rn


_EN = []


def _elastic_net_case(htable500):
    if not _EN:
        _EN.extend(B.elastic_net_case(htable500))
        for a in _EN:
            a.setflags(write=False)
    return _EN


@pytest.fixture
def ctx():
    from amico_amd import _capi
    return _capi.Context(-1)                                            # (closed when the last dictionary made on it is gone)


def _clean(ctx):
    st = ctx.last_stats()
    assert st['overflow_voxels'] == 0 and st['itercap_voxels'] == 0 and st['guard_trips'] == 0, st


# ------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('m,n', list(B.SUPPORT_CASES))
def test_supports_on_either_side_of_every_boundary(ctx, m, n):
    """supports inside the main pass (<= 16), inside the re-run pass (<= 48) and beyond it in ONE call -- with the tile in LDS (NR = 4: 200 x 60,
    NR = 2: 120 x 56) and read where it lies (the other shapes), the factor of k_batched_big in LDS and, for the largest supports of the two
    large shapes, in its global block"""
    from amico_amd import _capi
    A, y, xt, sizes, rn_ref = _support_case(m, n)
    dic = _capi.Dict(ctx, A, dense=True)
    assert dic.dense
    x, rn = _capi.nnls_batched(ctx, dic, y, return_rnorm=True)
    _clean(ctx)
    dense = ctx.last_dense()
    path = ctx.last_path()
    print('%d x %d: k_batched_big took %d of %d voxels, %.1f steps each; |x - x_true| %.2e, |rnorm - scipy| %.2e' % (
        m, n, dense['voxels'], len(y), dense['steps'] / max(1, dense['voxels']), np.abs(x - xt).max(), np.abs(rn - rn_ref).max()))
    assert np.array_equal(x > 0, xt > 0)
    assert np.abs(x - xt).max() < 1e-9
    assert np.abs(rn - rn_ref).max() < 1e-9
    assert 'k_batched_big' in path, path
    assert (sizes > 48).sum() <= dense['voxels'] <= (sizes > 20).sum(), dense
    xl = _capi.lasso_batched(ctx, dic, y, 1e-4, 1e-4)
    _clean(ctx)
    assert np.array_equal((xl > 0).sum(axis=1), sizes)
    assert (sizes > 48).sum() <= ctx.last_dense()['voxels'] <= (sizes > 20).sum()


# ------------------------------------------------------------------------------------------------------------- 2
def test_default_dictionaries_are_as_before(ctx):
    from amico_amd import _capi
    A, y, xt, sizes, _ = _support_case(200, 60)
    plain = _capi.Dict(ctx, A)
    assert not plain.dense
    with pytest.raises(_capi.AmxError) as e:
        _capi.nnls_batched(ctx, plain, y)
    assert e.value.code == _capi.AMX_E_OVERFLOW
    assert 'k_batched_big' not in ctx.last_path()
    small = sizes <= 48
    x0, rn0 = _capi.nnls_batched(ctx, plain, y[small], return_rnorm=True)
    _clean(ctx)
    assert ctx.last_dense()['voxels'] == 0 and 'k_batched_big' not in ctx.last_path()
    l0 = _capi.lasso_batched(ctx, plain, y[small], 1e-4, 1e-4)
    other = _capi.Context(-1)
    dic = _capi.Dict(other, A, dense=True)
    x1, rn1 = _capi.nnls_batched(other, dic, y[small], return_rnorm=True)
    _clean(other)
    assert other.last_dense()['voxels'] == 0 and 'k_batched_big' in other.last_path()          # (the one launch that finds a zero count)
    l1 = _capi.lasso_batched(other, dic, y[small], 1e-4, 1e-4)
    assert other.last_dense()['voxels'] == 0
    assert np.array_equal(x0, x1) and np.array_equal(rn0, rn1) and np.array_equal(l0, l1)      # bit for bit


# ------------------------------------------------------------------------------------------------------------- 3
def _kuhn_tucker(A2, idx, y, x, lam1, lam2):
    gp = gz = 0.0
    for d in range(A2.shape[0]):
        rows = np.flatnonzero(idx == d)
        G = (y[rows] - x[rows] @ A2[d].T) @ A2[d] - lam2 * x[rows] - lam1
        P = x[rows] > 0
        gp, gz = max(gp, np.abs(G[P]).max(initial=0.0)), max(gz, G[~P].max(initial=0.0))
    return gp, gz


@pytest.mark.parametrize('lam1,lam2', B.ELASTIC_NET_LAMBDAS)
def test_dense_elastic_net_on_nearly_collinear_atoms(ctx, htable500, lam1, lam2):
    """six NODDI stage-2 dictionaries (90 x 144): with a weak or no lambda1 the optimum holds up to ~100 of the 144 atoms"""
    from amico_amd import _capi
    from oracle import oracle
    A2, y, idx = _elastic_net_case(htable500)
    dic = _capi.Dict(ctx, A2, dense=True)
    x = _capi.lasso_batched(ctx, dic, y, lam1, lam2, idx)
    _clean(ctx)
    dense = ctx.last_dense()
    supp = (x > 0).sum(axis=1)
    gp, gz = _kuhn_tucker(A2, idx, y, x, lam1, lam2)
    print('lambda (%g, %g): supports %d .. %d, %d beyond 48; k_batched_big %d voxels, %.1f steps each; |g_P| %.2e, g_Z %.2e' % (
        lam1, lam2, supp.min(), supp.max(), int((supp > 48).sum()), dense['voxels'], dense['steps'] / max(1, dense['voxels']), gp, gz))
    assert x.min() >= 0.0 and 'k_batched_big' in ctx.last_path()
    assert dense['voxels'] >= (supp > 48).sum()
    if lam1 == 0.0:
        assert (supp > 48).any() and (supp <= 16).any()
    assert gp < 1e-9 and gz < 1e-9, (gp, gz)
    worst = 0.0
    for v in range(0, len(y), 5):
        worst = max(worst, np.abs(x[v] - oracle.lasso(A2[idx[v]], y[v], lam1, lam2)[0]).max())
    print('|x - oracle.lasso| %.2e' % worst)
    assert worst < 1e-7


# ------------------------------------------------------------------------------------------------------------- 4
def test_wide_dictionary_without_a_ridge(ctx):
    """60 x 100, lambda2 = 0: every support has m = 60 atoms and a zero residual; a block step that gathers more makes H_PP singular -- the
    rank guard.  x is not unique: compared are A x, the sign, the size of the support and the Kuhn-Tucker conditions"""
    from scipy.optimize import nnls as scipy_nnls
    from amico_amd import _capi
    A, y = B.wide_case()
    dic = _capi.Dict(ctx, A, dense=True)
    x, rn = _capi.nnls_batched(ctx, dic, y, return_rnorm=True)
    _clean(ctx)
    dense = ctx.last_dense()
    print('wide: k_batched_big %d voxels, %.1f steps each' % (dense['voxels'], dense['steps'] / max(1, dense['voxels'])))
    assert dense['voxels'] == len(y)
    assert x.min() >= 0.0 and ((x > 0).sum(axis=1) <= 60).all()
    for v in range(len(y)):
        xs, _ = scipy_nnls(A, y[v], maxiter=5000)
        assert np.abs(A @ x[v] - A @ xs).max() < 1e-8
        gp, gz = B.kuhn_tucker(A, y[v], x[v])
        bound = 1e-9 * max(1.0, np.linalg.norm(y[v]))
        assert gp < bound and gz < bound, (v, gp, gz)
        assert abs(rn[v] - np.linalg.norm(y[v] - A @ x[v])) < 1e-9


# ------------------------------------------------------------------------------------------------------------- 5
def test_scale_equivariance(ctx, htable500):
    from amico_amd import _capi
    A, y, xt, sizes, _ = _support_case(200, 60)
    A2, y2, idx = _elastic_net_case(htable500)
    dic, dic2 = _capi.Dict(ctx, A, dense=True), _capi.Dict(ctx, A2, dense=True)
    x1 = _capi.nnls_batched(ctx, dic, y)
    l1 = _capi.lasso_batched(ctx, dic, y, 1e-4, 1e-4)
    e1 = [_capi.lasso_batched(ctx, dic2, y2, a, b, idx) for a, b in B.ELASTIC_NET_LAMBDAS]
    for c in B.SCALES:
        xc = _capi.nnls_batched(ctx, dic, c * y)
        _clean(ctx)
        assert ctx.last_dense()['voxels'] >= (sizes > 48).sum()
        assert np.array_equal(xc > 0, x1 > 0) and np.abs(xc / c - x1).max() < 1e-9
        lc = _capi.lasso_batched(ctx, dic, c * y, 1e-4 * c, 1e-4)
        _clean(ctx)
        assert np.array_equal(lc > 0, l1 > 0) and np.abs(lc / c - l1).max() < 1e-9
        for (a, b), ref in zip(B.ELASTIC_NET_LAMBDAS, e1):
            ec = _capi.lasso_batched(ctx, dic2, c * y2, a * c, b, idx)
            _clean(ctx)
            print('scale %g, lambda (%g, %g): |x(c y) / c - x(y)| %.2e' % (c, a, b, np.abs(ec / c - ref).max()))
            assert np.array_equal(ec > 0, ref > 0) and np.abs(ec / c - ref).max() < 1e-9


# ------------------------------------------------------------------------------------------------------------- 6
def test_device_forms_match_the_host_forms(ctx):
    import ctypes as C
    import torch
    from amico_amd import _capi
    A, y, xt, sizes, _ = _support_case(200, 60)
    dic = _capi.Dict(ctx, A, dense=True)
    xh, rh = _capi.nnls_batched(ctx, dic, y, return_rnorm=True)
    lh = _capi.lasso_batched(ctx, dic, y, 1e-4, 1e-4)
    dev = torch.device('cuda', 0)
    yt = torch.from_numpy(np.array(y)).to(dev)
    xd = torch.empty((len(y), 60), dtype=torch.float64, device=dev)
    rd = torch.empty(len(y), dtype=torch.float64, device=dev)
    ld = torch.empty((len(y), 60), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    L, p = _capi.lib(), lambda t: C.c_void_p(t.data_ptr())
    ctx.check(L.amx_nnls_batched_device(ctx._h, dic._h, None, p(yt), len(y), p(xd), p(rd), None))
    ctx.sync()
    _clean(ctx)
    assert ctx.last_dense()['voxels'] >= (sizes > 48).sum()
    ctx.check(L.amx_lasso_batched_device(ctx._h, dic._h, None, p(yt), len(y), 1e-4, 1e-4, p(ld), None))
    ctx.sync()
    _clean(ctx)
    assert np.array_equal(xd.cpu().numpy(), xh) and np.array_equal(rd.cpu().numpy(), rh) and np.array_equal(ld.cpu().numpy(), lh)


# ------------------------------------------------------------------------------------------------------------- 7
def test_switching_dense_on_and_off(ctx):
    from amico_amd import _capi
    A, y, xt, sizes, _ = _support_case(200, 60)
    dic = _capi.Dict(ctx, A)
    dic.set_dense(True)
    dic.set_dense(True)                                                 # idempotent
    x1 = _capi.nnls_batched(ctx, dic, y)
    dic.set_dense(False)
    assert not dic.dense
    with pytest.raises(_capi.AmxError) as e:
        _capi.nnls_batched(ctx, dic, y)
    assert e.value.code == _capi.AMX_E_OVERFLOW
    dic.set_dense(False)
    dic.set_dense(True)
    assert dic.dense
    assert np.array_equal(_capi.nnls_batched(ctx, dic, y), x1)
    _clean(ctx)
    other = _capi.Context(-1)
    with pytest.raises(ValueError, match='not a dictionary of this ctx'):
        dic.set_dense(False, ctx=other)
    assert dic.dense                                                    # refused: nothing changed
    assert np.array_equal(_capi.nnls_batched(ctx, dic, y), x1)
