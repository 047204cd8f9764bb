"""The float64 reference of the LUT resampling GEMM and its bound (tests/lut_gemm_np.py), checked on the CPU before any kernel is held
to them: a float32 accumulation of the very shapes of the GPU test stays inside the bound of the reference, and the reference is the
numpy statement of lut.pyx:274-311 (oracle/lut_np.resample_kernel)."""
import numpy as np
import pytest

import lut_gemm_np as G
from oracle import lut_np


def _ids(shapes):
    return ['x'.join(map(str, s)) for s in shapes]


ALL = G.TILE + G.LDS + G.GENERIC


def test_the_table_of_shapes_is_complete():
    assert len(set(ALL)) == len(ALL)
    assert {n for _, k, n in G.TILE if k == 182} == {1, 31, 32, 33, 91, 92}
    assert all({m for m, k, n in G.TILE if k == 182 and n == nn} >= {1, 31, 33, 130, 360} for nn in (1, 31, 32, 33, 91, 92))
    assert {k for _, k, _ in G.TILE} == {88, 90, 92, 180, 182, 184, 252, 254, 256} and G.LARGE in G.TILE
    assert {k for _, k, _ in G.LDS} == {1, 2, 7, 91, 93, 183, 185, 255, 182}
    assert {m for m, _, _ in G.LDS} == {1, 33, 129}
    # K = 185 ... 255 take half-length 64: [64][258] floats are 66 KB, so N = 64 is admitted for every K of the list
    assert all((m, k, n) in G.LDS for k in (1, 2, 7, 91, 93, 183, 185, 255) for n in (1, 33, 64) for m in (1, 33, 129))
    assert len(G.FUSED) == 7 * 3 * 2


@pytest.mark.parametrize('shape', ALL, ids=_ids(ALL))
def test_float32_accumulation_stays_inside_the_bound(shape):
    M, K, N = shape
    L, Y, idx, nS = G.make_case(M, K, N, seed=1)
    assert L.dtype == Y.dtype == np.float32 and nS > N and len(set(idx.tolist())) == N and idx.max() < nS
    ref = G.resample_ref(L, Y, idx, nS)
    bound = G.resample_bound(L, Y)
    assert ref.dtype == np.float64 and bound.shape == (M, N)
    err = np.abs(G.f32_in_order(L, Y).astype(np.float64) - ref[:, idx])
    assert np.all(err <= bound), float((err / bound).max())
    other = np.setdiff1d(np.arange(nS), idx)
    assert np.all(ref[:, other] == 1.0)
    # the bound is a rounding bound, not a tolerance: a few ulp of the typical element
    assert np.median(bound) < 4 * (K + 2) * G.U * max(K, 1)


@pytest.mark.parametrize('case', G.FUSED[::5], ids=_ids(G.FUSED[::5]))
def test_fused_left_operand_is_rounded_once(case):
    Z, R, Y, idx, nS = G.make_fused_case(*case, seed=2)
    n_sh, shells, ndirs, atoms = case
    Lf = G.fused_left(Z, R)
    assert Lf.shape == (atoms * ndirs, n_sh * shells) and Lf.dtype == np.float32
    a, d, k = atoms - 1, ndirs // 2, n_sh * shells - 1
    assert Lf[a * ndirs + d, k] == np.float32(Z[a, k]) * np.float32(R[d, k % n_sh])
    exact = Z.astype(np.float64)[:, None, :] * np.tile(R.astype(np.float64), (1, shells))[None]
    assert np.all(np.abs(Lf.astype(np.float64) - exact.reshape(Lf.shape)) <= G.U * np.abs(exact.reshape(Lf.shape)))
    err = np.abs(G.f32_in_order(Lf, Y).astype(np.float64) - G.fused_ref(Z, R, Y, idx, nS)[:, idx])
    assert np.all(err <= G.fused_bound(Z, R, Y))


@pytest.mark.parametrize('shape', [(60, 182, 61), (33, 91, 31), (5, 455, 70)], ids=_ids([(60, 182, 61), (33, 91, 31), (5, 455, 70)]))
def test_reference_is_the_numpy_statement(shape):
    """resample_kernel on the same operands in float64 rounds its result once to float32: within one ulp of the reference, element
    by element, and the same ones outside idx_out"""
    M, K, N = shape
    L, Y, idx, nS = G.make_case(M, K, N, seed=3)
    ref = G.resample_ref(L, Y, idx, nS)
    KR = lut_np.resample_kernel(L.astype(np.float64), nS, idx, Y.astype(np.float64), False, M)
    assert KR.dtype == np.float32 and KR.shape == ref.shape
    assert np.all(np.abs(KR.astype(np.float64) - ref) <= G.U * np.abs(ref))
    iso = lut_np.resample_kernel(L[0].astype(np.float64), nS, idx, Y.astype(np.float64), True, M)
    assert np.all(np.abs(iso.astype(np.float64) - ref[0]) <= G.U * np.abs(ref[0]))
    # ... and the float32 statement itself (BLAS order) is inside the bound
    KR32 = lut_np.resample_kernel(L, nS, idx, Y, False, M)
    assert np.all(np.abs(KR32.astype(np.float64) - ref)[:, idx] <= G.resample_bound(L, Y))
