"""High-precision references of the tables the library builds on the device from an uploaded dictionary (the tiles' Gram matrices, the
ridge matrices H and their inverses, SANDI's row-space tables and MFMA operand, CylinderZeppelinBall's M, M 1, M A') and the properties a
compressed basis U must have, with the rounding bounds the GPU tests hold the fetched tables to (test_gpu_tables.py, test_tables_np.py).
Plain numpy in np.longdouble; where long double is no wider than double, exact rational arithmetic instead.  CPU only; nothing here
touches the library under test."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
WIDE = bool(np.finfo(LD).eps < 2.0 ** -52)
U53, U52 = 2.0 ** -53, 2.0 ** -52
KD, SCREEN_LD = 12, 192          # kSeedKD, kScreenLd (amx_kernels.hpp)


def matmul(X, Y):
    """X @ Y in long double (or exactly, then rounded once, where long double is double)"""
    X, Y = np.asarray(X), np.asarray(Y)
    if WIDE:
        return X.astype(LD) @ Y.astype(LD)
    Xf = [[Fraction(float(v)) for v in row] for row in np.atleast_2d(X)]
    Yf = [[Fraction(float(v)) for v in row] for row in np.atleast_2d(Y).T]
    out = np.array([[float(sum(a * b for a, b in zip(r, c))) for c in Yf] for r in Xf])
    return out.reshape(np.shape(X @ Y)).astype(LD)


def absmul(X, Y):
    """|X| @ |Y| in float64: the scale every product bound below multiplies"""
    return np.abs(np.asarray(X, dtype=np.float64)) @ np.abs(np.asarray(Y, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ Gram matrices, H, inverses
def gram(A, rows=None):
    """(G, S): G = A'A over the rows `rows` (all by default) and S[j][k] = sum_i |a_ij a_ik|.  A: [nS][n]"""
    A = np.asarray(A)
    if rows is not None:
        A = A[np.asarray(rows)]
    return matmul(A.T, A), absmul(A.T, A)


def gram_bound(S, n_terms):
    """|fl(sum of n exactly representable products) - sum| <= n 2^-53 sum |products| (products of float32 values are exact in float64;
    a fused multiply-add rounds no more often)"""
    return n_terms * U53 * S


def ridge(G, S, lam2, n_pad=None, pad_diag=1.0):
    """(H, S_H): H = G + lambda2 I on the dictionary, padded to n_pad with pad_diag on the diagonal; lambda2 counts as one more term"""
    n = G.shape[0]
    n_pad = n if n_pad is None else n_pad
    H = np.zeros((n_pad, n_pad), dtype=LD)
    SH = np.zeros((n_pad, n_pad))
    H[:n, :n] = G + LD(lam2) * np.eye(n, dtype=LD)
    SH[:n, :n] = S + abs(lam2) * np.eye(n)
    for k in range(n, n_pad):
        H[k, k] = pad_diag
    return H, SH


def inverse(H):
    """H^-1 in long double: numpy's float64 inverse, then Newton steps X <- X (2 I - H X) in long double"""
    H = np.asarray(H, dtype=LD)
    X = np.linalg.inv(H.astype(np.float64)).astype(LD)
    I2 = 2 * np.eye(H.shape[0], dtype=LD)
    for _ in range(3):
        X = matmul(X, I2 - matmul(H, X))
    return X


def cond2(H):
    s = np.linalg.svd(np.asarray(H, dtype=np.float64), compute_uv=False)
    return float(s[0] / s[-1])


def inverse_residual(H, X):
    """max |H X - I| in long double"""
    H = np.asarray(H, dtype=LD)
    return float(np.abs(matmul(H, X) - np.eye(H.shape[0], dtype=LD)).max())


def inverse_bound(H):
    """||H X - I||_max <= 8 n 2^-52 cond2(H) for an inverse X computed in float64 by a stable method"""
    return 8.0 * H.shape[0] * U52 * cond2(H)


def product_bound(X, Y, n_terms=None):
    """|fl(X Y) - X Y| <= n 2^-52 |X| |Y| elementwise (n: the length of the sums)"""
    n_terms = np.shape(X)[-1] if n_terms is None else n_terms
    return n_terms * U52 * absmul(X, Y)


# ------------------------------------------------------------------------------------------------ tiles
def noddi_atoms(K, d, exvivo=False):
    """float32 [nS][n_atoms] of orientation d as the tiles hold it: wm, (a column of ones), iso"""
    cols = [K['wm'][:, d, :].astype(np.float32)]
    if exvivo:
        cols.append(np.ones((1, K['iso'].shape[0]), dtype=np.float32))
    cols.append(np.asarray(K['iso'], dtype=np.float32)[None, :])
    return np.ascontiguousarray(np.concatenate(cols, axis=0).T)


def tile_layout(A, ldA, tile_stride):
    """one orientation's tile: tile[i * ldA + j] = A[i][j], zeros elsewhere"""
    nS, n = A.shape
    t = np.zeros(tile_stride, dtype=A.dtype)
    t[:nS * ldA].reshape(nS, ldA)[:, :n] = A
    return t


def lda_of(n_atoms):
    return n_atoms if n_atoms & 1 else n_atoms + 1


def tile_stride_of(nS, n_atoms):
    return (nS * lda_of(n_atoms) + 3) & ~3


# ------------------------------------------------------------------------------------------------ compressed bases
def basis_defect(U):
    """(diag, off): the diagonal of U'U and the largest |off-diagonal entry| in long double"""
    UtU = matmul(np.asarray(U).T, U)
    d = np.diag(UtU).astype(np.float64)
    off = UtU - np.diag(np.diag(UtU))
    return d, float(np.abs(off).max())


def residual_columns(U, A):
    """E = A - U (U'A) in long double, [nS][n]"""
    A = np.asarray(A).astype(LD)
    return A - matmul(U, matmul(np.asarray(U).T, A))


def column_norms(E):
    E = np.asarray(E, dtype=LD)
    return np.sqrt((E * E).sum(axis=0)).astype(np.float64)


def screen_values(Sf, Utr):
    """the solver's compressed dual values (amx_solver.hpp, NNSolver::certify_seed): float32 sums over d in ascending order of
    Sf[d][j] * float32((U'r)_d).  Sf: float32 [KD][n], Utr: float64 [KD][n_r] -> float32 [n][n_r]"""
    Sf = np.asarray(Sf, dtype=np.float32)
    ut = np.zeros((Sf.shape[1], Utr.shape[1]), dtype=np.float32)
    for d in range(Sf.shape[0]):
        ut = (ut + (Sf[d][:, None] * Utr[d].astype(np.float32)[None, :]).astype(np.float32)).astype(np.float32)
    return ut


def screen_slack(A, U, Sf, kappa, R):
    """min over atoms j and test vectors r (the columns of R [nS][n_r]) of ut_j + 1.0625 kappa ||r|| - a_j'r: negative = the screen
    could skip an atom whose dual value is positive"""
    R = np.asarray(R, dtype=np.float64)
    Utr = matmul(np.asarray(U).T, R).astype(np.float64)
    ut = screen_values(Sf, Utr).astype(np.float64)
    exact = matmul(np.asarray(A).T, R).astype(np.float64)
    rn = np.sqrt((R.astype(LD) ** 2).sum(axis=0)).astype(np.float64)
    return float((ut + 1.0625 * kappa * rn[None, :] - exact).min())


# ------------------------------------------------------------------------------------------------ SANDI
def sandi_row_tables(A, lam1, lam2):
    """the row-space tables of a [M][N] SANDI dictionary (amx_sandi_lane.hip): T[j][i (i + 1) / 2 + k] = a_ij a_kj (k <= i),
    W = (lambda2 I + A A')^-1, G = A'W [N][M], g0 = -(lambda1 / lambda2) (1 - A'W A 1); also B = lambda2 I + A A'"""
    A = np.asarray(A, dtype=np.float64)
    M, N = A.shape
    T = np.zeros((N, M * (M + 1) // 2))
    for i in range(M):
        for k in range(i + 1):
            T[:, i * (i + 1) // 2 + k] = A[i] * A[k]            # one rounding, as in the kernel
    B = matmul(A, A.T) + LD(lam2) * np.eye(M, dtype=LD)
    W = inverse(B)
    G = matmul(A.T, W)
    g0 = -(LD(lam1) / LD(lam2)) * (1 - matmul(G, matmul(A, np.ones((N, 1))))[:, 0])
    return dict(T=T, B=B, W=W, G=G, g0=g0)


def sl_volume(s, q):
    """volume that K step s of lane quarter q reads (amx_sandi_long.hip)"""
    return 16 * (s >> 2) + 4 * q + (s & 3)


def sandi_long_operand(A, NP, KS):
    """A' in MFMA operand order: [(mt KS + s) 64 + l] = A[sl_volume(s, l / 16)][16 mt + l % 16], zero beyond the dictionary"""
    nS, n = A.shape
    out = np.zeros((NP // 16) * KS * 64)
    for mt in range(NP // 16):
        for s in range(KS):
            for l in range(64):
                atom, i = 16 * mt + (l & 15), sl_volume(s, l >> 4)
                if i < nS and atom < n:
                    out[(mt * KS + s) * 64 + l] = A[i, atom]
    return out


# ------------------------------------------------------------------------------------------------ CylinderZeppelinBall
def czb_split(tab, nSp):
    """one orientation's table -> M [32][33], H [32][33], m1 [32], B [32][nSp], At [32][nSp]"""
    o = 0
    M = tab[o:o + 32 * 33].reshape(32, 33); o += 32 * 33
    H = tab[o:o + 32 * 33].reshape(32, 33); o += 32 * 33
    m1 = tab[o:o + 32]; o += 32
    B = tab[o:o + 32 * nSp].reshape(32, nSp); o += 32 * nSp
    At = tab[o:o + 32 * nSp].reshape(32, nSp); o += 32 * nSp
    assert o == tab.size
    return M, H, m1, B, At


def fw_split(tab, nS, N):
    """one orientation's FreeWater table -> A [nS][NP], H^-1 [N][NP], H [N][N]"""
    NP = (N + 1) & ~1
    o = 0
    A = tab[o:o + nS * NP].reshape(nS, NP); o += nS * NP
    Hi = tab[o:o + N * NP].reshape(N, NP); o += N * NP
    H = tab[o:o + N * N].reshape(N, N); o += N * N
    assert tab.size == (o + 1) & ~1
    return A, Hi, H


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
# (shared with test_tables_np.py, which checks on the CPU what the bounds of test_gpu_tables.py rely on)
N_ORI = 5
FW_ATOMS = (10, 11, 12)                     # k_fw_orient_prep<11>, <11>, <12>
FW_LAM2 = (1e-3, 5e-3)
CZB_SHAPES = ((26, 99), (26, 100), (26, 101), (26, 160), (12, 99), (12, 160))      # (atoms, volumes): nSp 100 / 160
CZB_LAM2 = (4.0, 1e-2)                      # the model's default and the gate of the fast path
SANDI_ROWS_LAMBDAS = ((0.0, 5e-3), (0.25, 5e-3), (0.25, 1e-3))
SANDI_LONG_SHAPES = ((129, 15), (144, 17), (145, 15))
SANDI_LONG_LAM2 = (5e-3, 1e-3)
_CACHE = {}


def orientations():
    from amico_amd import synthetic as S
    if 'ori' not in _CACHE:
        dirs = S.fibonacci_hemisphere(N_ORI)
        _CACHE['ori'] = (dirs, S.build_htable(dirs))
    return _CACHE['ori']


def fw_scheme():
    from amico_amd import synthetic as S
    return S.make_scheme(n_b0=3, shells=((700.0, 12), (2000.0, 18)), seed=4)        # 33 volumes


def fw_kernels(n_atoms):
    from amico_amd import synthetic as S
    if ('fw', n_atoms) not in _CACHE:
        _CACHE['fw', n_atoms] = S.freewater_kernels(fw_scheme(), orientations()[0], d_perps=np.linspace(0.1, 1.0, n_atoms - 1) * 1e-3)
    return _CACHE['fw', n_atoms]


def fw_atoms(K, d):
    return np.ascontiguousarray(np.concatenate([K['D'][:, d, :], K['CSF']], axis=0).T.astype(np.float32))


def czb_kernels(n_atoms, nS):
    import czb_np as Z
    if ('czb', n_atoms, nS) not in _CACHE:
        Rs, d_perps, d_isos = Z.atom_sets(n_atoms)
        K = Z.czb_kernels(Z.make_scheme(nS, seed=nS), range(N_ORI), Rs, d_perps, d_isos, 0.6e-3, lut_dirs=orientations()[0], ndirs=N_ORI)
        _CACHE['czb', n_atoms, nS] = (K, Rs)
    return _CACHE['czb', n_atoms, nS]


def czb_atoms(K, d):
    return np.ascontiguousarray(np.concatenate([K['wmr'][:, d], K['wmh'][:, d], K['iso']], axis=0).T.astype(np.float32))


def sandi_dictionary(nS, n_atoms, seed=0):
    """a SANDI-like dictionary of unit columns, float64 [nS][n_atoms]: decays exp(-b D_j) over nS b-values, plus a little
    structure per volume so that no two columns are parallel; (kernels dict, Rs, d_in, d_isos) as upload_sandi takes them"""
    rng = np.random.default_rng(seed + 1000 * nS + n_atoms)
    b = np.sort(rng.uniform(0.0, 8.0, nS))
    D = np.geomspace(0.05, 3.0, n_atoms)
    A = np.exp(-np.outer(b, D)) * (1.0 + 0.05 * rng.standard_normal((nS, n_atoms)))
    norms = 1.0 / np.linalg.norm(A, axis=0)
    A = A * norms
    n_rs = n_atoms // 3
    n_in = n_atoms // 3
    n_iso = n_atoms - n_rs - n_in
    K = {'model': 'SANDI', 'signal': np.asfortranarray(A), 'norms': norms}
    return K, np.linspace(1e-6, 12e-6, n_rs), np.linspace(0.25e-3, 3e-3, n_in), np.linspace(0.25e-3, 3e-3, n_iso)


def inverse_inputs():
    """(label, H) of every matrix whose device inverse test_gpu_tables.py bounds by inverse_bound: long double, unpadded"""
    for n in FW_ATOMS:
        K = fw_kernels(n)
        for lam2 in FW_LAM2:
            for d in range(N_ORI):
                G, S = gram(fw_atoms(K, d))
                yield 'FreeWater %d atoms lambda2 %g dir %d' % (n, lam2, d), ridge(G, S, lam2)[0]
    for n, nS in CZB_SHAPES:
        K, _ = czb_kernels(n, nS)
        for lam2 in CZB_LAM2:
            for d in range(N_ORI):
                G, S = gram(czb_atoms(K, d))
                yield 'CZB %d atoms %d volumes lambda2 %g dir %d' % (n, nS, lam2, d), ridge(G, S, lam2)[0]
    K = sandi_dictionary(6, 15)[0]
    for lam1, lam2 in SANDI_ROWS_LAMBDAS:
        yield 'SANDI rows lambda2 %g' % lam2, sandi_row_tables(np.asarray(K['signal']), lam1, lam2)['B']


# NODDI dictionaries, one per branch of the upload (amx_lut.hip, amx_seed.hip): name -> what noddi_case builds
NODDI_SHAPES = ('bench', 'v150', 'v288', 'exvivo', 'single_b0', 'nonunit_b0', 'grid3x3', 'atoms5', 'v10', 'dup3', 'noseed')
LDS_PER_CU = 160 * 1024          # kLdsPerCU (amx_noddi_route.hpp)


def noddi_branches(nS, n_atoms):
    """the branches an upload of this shape takes, restated from amx_lut.hip / amx_seed.hip"""
    ldA = lda_of(n_atoms)
    return dict(gram_in_lds=nS * ldA * 4 <= 160 * 1024, basis_in_lds=(nS * ldA + KD * nS + 256) * 8 <= LDS_PER_CU, seeds=n_atoms <= 160)


def noddi_case(name):
    """(K, scheme, exvivo) of the NODDI dictionary `name` on the N_ORI orientations"""
    from amico_amd import synthetic as S
    if ('noddi', name) in _CACHE:
        return _CACHE['noddi', name]
    dirs = orientations()[0]
    grid = {}
    sch = S.make_scheme(seed=0)                                                          # 99 volumes, 9 b0
    if name == 'v150':
        sch = S.make_scheme(n_b0=10, shells=((700.0, 60), (2000.0, 80)), seed=1)
    elif name == 'v288':
        sch = S.make_scheme(n_b0=18, shells=((700.0, 90), (2000.0, 180)), seed=2)
    elif name == 'single_b0':
        sch = S.make_scheme(n_b0=1, shells=((700.0, 30), (2000.0, 60)), seed=3)
    elif name == 'v10':
        sch = S.make_scheme(n_b0=1, shells=((700.0, 4), (2000.0, 5)), seed=5)
    elif name in ('grid3x3', 'dup3'):
        grid = dict(IC_VFs=np.linspace(0.1, 0.99, 3), IC_ODs=np.array([0.03, 0.5, 0.99]))
    elif name == 'atoms5':
        grid = dict(IC_VFs=np.array([0.3, 0.8]), IC_ODs=np.array([0.06, 0.6]))
    elif name == 'noseed':
        grid = dict(IC_VFs=np.linspace(0.1, 0.99, 13), IC_ODs=np.linspace(0.03, 0.99, 13))
    K = S.noddi_kernels(sch, dirs, **grid)
    if name == 'nonunit_b0':
        K['wm'][3, :, sch.b0_idx[1]] = np.float32(0.999)                                 # one atom, one b0 row
    if name == 'dup3':                                                                   # three atoms, each twice, and iso: rank 4
        sel = [0, 4, 8, 0, 4, 8]
        K = dict(K, wm=K['wm'][sel].copy(), kappa=K['kappa'][sel].copy(), icvf=K['icvf'][sel].copy(), norms=K['norms'][:, sel].copy())
    _CACHE['noddi', name] = (K, sch, name == 'exvivo')
    return _CACHE['noddi', name]
