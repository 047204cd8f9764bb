"""The LUT resampling GEMM (amx_lut_resample / amx_lut_rotate_resample, csrc/amx_lut_gemm.hip) held to its float64 reference on all three
kernels: every case first asserts the kernel it is about (amx_lut_route), then

 * bound: EVERY element within (K + 2) 2^-24 (|L| |Y|^T) of the float64 product (tests/lut_gemm_np.py; K + 3 for the fused call), the
   columns outside idx_out exactly 1.0;
 * probes, bit for bit: an identity left operand returns the operator itself, a one-hot operator returns columns of the left operand --
   every reduction index of every row of either operand is read from where it belongs (a sum of exact zeros and one product by 1.0);
 * the fused (zonal x basis) call against the same bound, its refusal, and against the plain call on the tile kernel;
 * NODDI.resample on a protocol with an odd number of DWI volumes, atom by atom.

Each test prints `lut_gemm_ratio <route> <shape> <max |got - ref| / bound>` (pytest -s) for DESIGN.md's record."""
import numpy as np
import pytest

import lut_gemm_np as G
from amico_amd import _capi, lut

pytestmark = pytest.mark.gpu


def _ids(shapes):
    return ['x'.join(map(str, s)) for s in shapes]


def _route(K, N, fused=False):
    return _capi.lut_route(K, N, fused)['route']


def _hold(got, ref, bound, idx, nS, tag):
    """every element of got[:, idx] within bound of ref, everything else exactly one"""
    assert got.dtype == np.float32 and got.shape == ref.shape
    other = np.setdiff1d(np.arange(nS), idx)
    assert other.size and np.all(got[:, other] == 1.0)
    err = np.abs(got[:, idx].astype(np.float64) - ref[:, idx])
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    print(f'lut_gemm_ratio {tag} {ratio:.4f}')
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, (tag, len(bad), bad[:8].tolist(), ratio)


def _bound_case(shape, route):
    M, K, N = shape
    assert _route(K, N) == route, (shape, _capi.lut_route(K, N))          # the kernel this case is about
    L, Y, idx, nS = G.make_case(M, K, N, seed=11)
    got = lut.resample_kernels(L, nS, idx, Y)
    _hold(got, G.resample_ref(L, Y, idx, nS), G.resample_bound(L, Y), idx, nS, f'{route} {M}x{K}x{N}')


# ---- a. every element within the rounding bound, per kernel
@pytest.mark.parametrize('shape', G.TILE, ids=_ids(G.TILE))
def test_tile_kernel_within_the_bound(shape):
    _bound_case(shape, 'tile')


@pytest.mark.parametrize('shape', G.LDS, ids=_ids(G.LDS))
def test_lds_kernel_within_the_bound(shape):
    _bound_case(shape, 'lds')


@pytest.mark.parametrize('shape', G.GENERIC, ids=_ids(G.GENERIC))
def test_generic_kernel_within_the_bound(shape):
    _bound_case(shape, 'generic')


# ---- b. probes, bit for bit.  (route, K, N): three K of the tile kernel whose K / 2 is odd -- with N odd the operator ends 8 bytes into
# a 16-byte piece of its staging copy -- and one odd and one even K for each of the other two kernels
PROBES = [('tile', 90, 33), ('tile', 182, 31), ('tile', 182, 91), ('tile', 182, 32), ('tile', 254, 7),
          ('lds', 91, 33), ('lds', 182, 93), ('generic', 257, 5), ('generic', 258, 33)]


@pytest.mark.parametrize('route,K,N', PROBES, ids=['-'.join(map(str, p)) for p in PROBES])
def test_operator_probe_identity_left_operand(route, K, N):
    """L = the K x K identity: out[:, idx] is the operator transposed, exactly"""
    assert _route(K, N) == route
    _, Y, idx, nS = G.make_case(K, K, N, seed=12)
    got = lut.resample_kernels(np.eye(K, dtype=np.float32), nS, idx, Y)
    wrong = np.argwhere(got[:, idx] != Y.T)
    assert wrong.size == 0, ('(k, n) of operator entries read from elsewhere', wrong[:8].tolist())
    assert np.all(got[:, np.setdiff1d(np.arange(nS), idx)] == 1.0)


@pytest.mark.parametrize('M', (1, 33, 131))
@pytest.mark.parametrize('route,K,N', PROBES, ids=['-'.join(map(str, p)) for p in PROBES])
def test_left_operand_probe_one_hot_operator(route, K, N, M):
    """operator row n = the unit vector of reduction index K - N + n, M odd (a last row tile with an odd number of rows):
    out[m, idx[n]] is L[m, K - N + n], exactly"""
    assert _route(K, N) == route and N <= K
    L, _, idx, nS = G.make_case(M, K, N, seed=13)
    Y = np.zeros((N, K), dtype=np.float32)
    Y[np.arange(N), K - N + np.arange(N)] = 1.0
    got = lut.resample_kernels(L, nS, idx, Y)
    wrong = np.argwhere(got[:, idx] != L[:, K - N:])
    assert wrong.size == 0, ('(m, n) of left-operand entries read from elsewhere', wrong[:8].tolist())
    assert np.all(got[:, np.setdiff1d(np.arange(nS), idx)] == 1.0)


# ---- c. the fused call
@pytest.mark.parametrize('case', G.FUSED, ids=_ids(G.FUSED))
def test_fused_within_the_bound(case):
    n_sh, shells, ndirs, atoms = case
    K = n_sh * shells
    assert _route(K, G.FUSED_N, fused=True) == 'lds'
    Z, R, Y, idx, nS = G.make_fused_case(*case, seed=14)
    got = _capi.lut_rotate_resample(_ctx(), Z, R, Y, idx, nS)
    assert got.shape == (atoms, ndirs, nS)
    _hold(got.reshape(atoms * ndirs, nS), G.fused_ref(Z, R, Y, idx, nS), G.fused_bound(Z, R, Y), idx, nS,
          f'fused {n_sh}x{shells} dirs {ndirs} atoms {atoms}')


def _ctx():
    from amico_amd.models import get_context
    return get_context()


def test_fused_beyond_256_reduction_indices_is_refused():
    assert _route(273, G.FUSED_N, fused=True) == 'refused'
    Z, R, Y, idx, nS = G.make_fused_case(91, 3, 33, 1, seed=15)
    with pytest.raises(ValueError, match=r'amx_lut_rotate_resample: shape beyond the fused kernel \(K <= 256, operator <= 80 KB\)'):
        _capi.lut_rotate_resample(_ctx(), Z, R, Y, idx, nS)
    # the context is as good as before
    got = _capi.lut_rotate_resample(_ctx(), Z[:, :182], R, Y[:, :182], idx, nS)
    _hold(got.reshape(33, nS), G.fused_ref(Z[:, :182], R, Y[:, :182], idx, nS), G.fused_bound(Z[:, :182], R, Y[:, :182]), idx, nS,
          'fused after a refusal')


@pytest.mark.parametrize('n_sh,shells', [(91, 2), (45, 2)])
@pytest.mark.parametrize('ndirs', (33, 500))
def test_fused_equals_the_plain_call_on_the_tile_kernel(n_sh, shells, ndirs):
    """the shapes of the fused table whose K is on the tile kernel's list: the lds kernel with the left operand formed in registers and
    the tile kernel with the same operand from memory differ by no more than the sum of their bounds"""
    K = n_sh * shells
    assert _route(K, G.FUSED_N, fused=True) == 'lds' and _route(K, G.FUSED_N) == 'tile'
    Z, R, Y, idx, nS = G.make_fused_case(n_sh, shells, ndirs, 3, seed=16)
    fused = _capi.lut_rotate_resample(_ctx(), Z, R, Y, idx, nS).reshape(3 * ndirs, nS)
    Lf = G.fused_left(Z, R)
    plain = lut.resample_kernels(Lf, nS, idx, Y)
    diff = np.abs(fused.astype(np.float64) - plain.astype(np.float64))[:, idx]
    assert np.all(diff <= G.fused_bound(Z, R, Y) + G.resample_bound(Lf, Y))
    assert np.array_equal(fused[:, np.setdiff1d(np.arange(nS), idx)], plain[:, np.setdiff1d(np.arange(nS), idx)])


# ---- d. through the product: NODDI's dictionary on a protocol with an odd number of DWI volumes
def test_noddi_resample_with_an_odd_number_of_volumes():
    """two shells of 21 + 40 directions: K = 182, N = 61 on the tile kernel, where the operator's staging copy ends inside a 16-byte
    piece.  lut_np.resample_kernel on the same float32 operands, summed in float64 and rounded once, is the reference"""
    from amico_amd import models, synthetic as S
    from oracle import lut_np
    scheme = S.make_scheme(n_b0=3, shells=((700.0, 21), (2000.0, 40)))
    lut_dirs = S.fibonacci_hemisphere(60)
    aux = lut.aux_matrices(12, lut_dirs)
    idx_in, idx_o = lut.aux_structures_generate(scheme, 12)
    hr = lut.high_resolution_scheme(scheme, aux['grad'])
    m = models.NODDI()
    m.set(IC_VFs=np.array([0.3, 0.7]), IC_ODs=np.array([0.1, 0.5, 0.9]))
    m.scheme = scheme
    Kz = S.noddi_kernels(hr, np.array([[0.0, 0.0, 1.0]]), IC_VFs=m.IC_VFs, IC_ODs=m.IC_ODs)
    lms = [lut.rotate_kernel(Kz['wm'][a, 0].astype(np.float64), aux, idx_in, idx_o, False, 60) for a in range(6)]
    lms.append(lut.rotate_kernel(Kz['iso'].astype(np.float64), aux, idx_in, idx_o, True, 60))
    idx_out, ylm_out = lut.aux_structures_resample(scheme, 12)
    assert ylm_out.shape == (61, 182) and ylm_out.dtype == np.float32 and all(a.dtype == np.float32 for a in lms)
    assert _route(182, 61) == 'tile'
    K = m.resample(lms, idx_out, ylm_out, False, 60)
    assert K['wm'].shape == (6, 60, scheme.nS)
    y64 = ylm_out.astype(np.float64)
    for a in range(6):
        ref = lut_np.resample_kernel(lms[a].astype(np.float64), scheme.nS, idx_out, y64, False, 60)
        _hold(K['wm'][a], ref.astype(np.float64), G.resample_bound(lms[a], ylm_out), idx_out, scheme.nS, f'tile NODDI atom {a}')
    ref = lut_np.resample_kernel(lms[6].astype(np.float64), scheme.nS, idx_out, y64, True, 60)
    _hold(K['iso'][None], ref.astype(np.float64)[None], G.resample_bound(lms[6][None], ylm_out), idx_out, scheme.nS, 'tile NODDI iso')
