"""numpy statement of the LUT resampling GEMM (include/amico_amd.h: amx_lut_resample / amx_lut_rotate_resample) in float64, its float32
rounding bound, and the table of shapes the GPU test holds the three kernels to (tests/test_gpu_lut_gemm.py; test infrastructure only).

The GEMM is out[m, idx[n]] = sum_k L[m, k] * Y[n, k] in float32 on the matrix cores, ones elsewhere.  Whatever the order of the K
fused multiply-adds (the kernels split K between the two halves of a wavefront and add the halves inside the MFMA), the computed sum
of K float32 products obeys  |fl(sum) - sum| <= gamma_K * sum_k |L[m, k]| |Y[n, k]|,  gamma_K = K u / (1 - K u), u = 2^-24: each
product is exact inside the FMA and a term passes through at most K roundings.  (K + 2) u is above gamma_K + u for every K here
(K <= 500: K^2 u^2 << u) and leaves the one rounding of the float64 reference to float32 no room to matter.  The fused call forms
its left operand with one more float32 rounding: K + 3.
"""
import numpy as np

U = 2.0 ** -24


def resample_ref(L, Y, idx, nS):
    """float64 product of the float32 inputs, scattered into ones -> float64 [M, nS]"""
    L = np.asarray(L, dtype=np.float32).astype(np.float64)
    Y = np.asarray(Y, dtype=np.float32).astype(np.float64)
    out = np.ones((L.shape[0], int(nS)), dtype=np.float64)
    out[:, np.asarray(idx)] = L @ Y.T
    return out


def resample_bound(L, Y, extra=2):
    """(K + extra) 2^-24 (|L| |Y|^T) -> float64 [M, N]"""
    L = np.abs(np.asarray(L, dtype=np.float32).astype(np.float64))
    Y = np.abs(np.asarray(Y, dtype=np.float32).astype(np.float64))
    return (L.shape[1] + extra) * U * (L @ Y.T)


def fused_left(Z, R):
    """the left operand of the fused call, as the kernel forms it: row (atom a, orientation d) is float32(Z[a, k]) *
    float32(R[d, k mod n_sh]) rounded once to float32 -> float32 [n_atoms * ndirs, K]"""
    Z = np.asarray(Z, dtype=np.float32)
    R = np.asarray(R, dtype=np.float32)
    shells = Z.shape[1] // R.shape[1]
    L = Z[:, None, :] * np.tile(R, (1, shells))[None, :, :]           # float32 x float32 -> float32: one rounding
    assert L.dtype == np.float32
    return L.reshape(-1, Z.shape[1])


def fused_ref(Z, R, Y, idx, nS):
    return resample_ref(fused_left(Z, R), Y, idx, nS)


def fused_bound(Z, R, Y):
    return resample_bound(fused_left(Z, R), Y, extra=3)


def f32_in_order(L, Y):
    """the same product accumulated in float32, k = 0, 1, 2 ... (numpy rounds every multiply and every add: two roundings per term
    where an FMA has one, still inside the bound) -> float32 [M, N]"""
    L = np.asarray(L, dtype=np.float32)
    Y = np.asarray(Y, dtype=np.float32)
    acc = np.zeros((L.shape[0], Y.shape[0]), dtype=np.float32)
    for k in range(L.shape[1]):
        acc += L[:, k, None] * Y[None, :, k]
    return acc


def make_case(M, K, N, seed):
    """N(0, 1) float32 operands, nS > N, idx a random unsorted subset of range(nS) -> (L, Y, idx, nS)"""
    rng = np.random.default_rng([seed, M, K, N])
    L = rng.standard_normal((M, K), dtype=np.float32)
    Y = rng.standard_normal((N, K), dtype=np.float32)
    nS = N + 1 + (M + K) % 7
    idx = rng.permutation(nS)[:N].astype(np.int32)
    return L, Y, idx, nS


# ---- the shapes (M, K, N) by the route they must take (amx_lut_route; every GPU case asserts it)
LARGE = (33893, 182, 91)      # at 256 CUs: 1060 row tiles over 1024 wavefronts -- one whole-tile round, 36 left-over tiles cut into their
#                               three column blocks, and a last tile of 5 rows

TILE = ([(m, 182, n) for n in (1, 31, 32, 33, 91, 92) for m in (1, 31, 33, 130, 360)]
        + [(65, 90, 33), (65, 90, 312)]
        + [(65, k, 33) for k in (88, 92, 180, 184)]
        + [(65, 254, 7), (65, 256, 30), (65, 252, 30)]
        + [LARGE])


def lds_admits(K, N):
    """the lds route's own size check, restated (K <= 256, operator padded to [N up to 32][4 kh2 + 2] floats within 80 KB)"""
    kh2 = 23 if K <= 92 else 46 if K <= 184 else 64
    return K <= 256 and -(-N // 32) * 32 * (4 * kh2 + 2) * 4 <= 80 * 1024


LDS = ([(m, k, n) for k in (1, 2, 7, 91, 93, 183, 185, 255) for n in (1, 33, 64) if lds_admits(k, n) for m in (1, 33, 129)]
       + [(m, 182, n) for n in (93, 96) for m in (1, 33, 129)])

GENERIC = [(130, 455, 300), (33, 257, 5), (65, 182, 97), (1, 273, 270), (33, 258, 40)]

FUSED = [(n_sh, shells, ndirs, atoms) for (n_sh, shells) in ((91, 1), (91, 2), (45, 2), (28, 3), (15, 4), (6, 1), (1, 1))
         for ndirs in (1, 33, 500) for atoms in (1, 3)]
FUSED_N = 33                  # volumes of the fused cases: one whole column block and a block of one


def make_fused_case(n_sh, shells, ndirs, atoms, seed, N=FUSED_N):
    rng = np.random.default_rng([seed, n_sh, shells, ndirs, atoms])
    K = n_sh * shells
    Z = rng.standard_normal((atoms, K), dtype=np.float32)
    R = rng.standard_normal((ndirs, n_sh), dtype=np.float32)
    Y = rng.standard_normal((N, K), dtype=np.float32)
    nS = N + 3
    idx = rng.permutation(nS)[:N].astype(np.int32)
    return Z, R, Y, idx, nS
