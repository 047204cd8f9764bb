"""FreeWater and SANDI in plain numpy, for the hard-voxel tests of their GPU routes (test_small_hard.py, test_gpu_small_hard.py): the
adversarial signal mix, the per-voxel Kuhn-Tucker certificate with a long-double residual, the map formulas of models.pyx:1240-1262
and 1570-1612, the error maps from long-double residuals and the dictionaries of the route table.  CPU only; nothing here touches
the library under test.  The high-precision re-solve is czb_np.czb_resolve (any dictionary), imported, not copied."""
import functools

import numpy as np

import czb_np as Z

LD = np.longdouble

KINDS = ('all zero', 'one atom', 'iso atom', 'pure noise', 'negated', 'first + last', 'signed', 'constant 1', 'uniform mixture',
         'one atom (1 + 2^-40)', 'as it is')
UP, DOWN = 2.0 ** 20, 2.0 ** -20


# ------------------------------------------------------------------------------------------------ signals
def hard_mix(A, y, seed, exact=True):
    """y [n, nS] (voxels of ONE dictionary A [nS, n_atoms]) with every third voxel overwritten -- v % 3 == 0, kind (v // 3) % 11
    indexing KINDS -- so that every wavefront holds hard and easy voxels:
      all zero | exactly one random atom | exactly the last (isotropic) atom | pure noise |N(0, 1)| | every sample negated (optimum
      x = 0) | the mean of the first and the last atom | signed samples (y + N(0, 0.3)) | constant 1 | the uniform mixture A 1 / n |
      one atom times 1 + 2^-40 | the voxel as it is.
    Then voxel v is multiplied by 2^20 if v % 5 == 1 and by 2^-20 if v % 5 == 3 (exact in float32 and float64, far from the 1e-16
    guards of the maps).  Returns (y, kind): a new float64 array; kind [n] is 10 ('as it is') for the voxels left alone.

    exact=False is for SANDI with a ridge of 1e-9 or less.  Its dictionaries have rank <= shells + 1 < n_atoms, so a signal that lies
    INSIDE the cone of the atoms -- one atom that is no extreme ray, the uniform mixture, one atom times 1 + 2^-40 -- has a whole face
    of optimal x, from which such a ridge picks one to a few digits only: the maps of the oracle and of the long-double re-solve,
    whose Kuhn-Tucker residuals are both below 1e-13, then differ by up to 1e-5 (against < 3e-10 at lambda2 = 2e-6; 'iso atom' and
    'first + last' lie on the boundary of the cone and agree to 1e-12 at any ridge).  The maps of those three kinds are ill-posed there,
    so they get noise of 0.02 added and the magnitude taken, as a measured voxel has; FreeWater's dictionaries have full column rank
    and keep them exact at every ridge."""
    A = np.asarray(A, dtype=np.float64)
    y = np.array(y, dtype=np.float64, copy=True)
    n, nS = y.shape
    n_atoms = A.shape[1]
    rng = np.random.default_rng(seed)
    v = np.arange(n)
    kind = np.where(v % 3 == 0, (v // 3) % 11, 10)

    def rows(k):
        return np.flatnonzero((v % 3 == 0) & (kind == k))
    y[rows(0)] = 0.0
    r = rows(1)
    y[r] = A[:, rng.integers(n_atoms, size=len(r))].T
    y[rows(2)] = A[:, -1]
    r = rows(3)
    y[r] = np.abs(rng.standard_normal((len(r), nS)))
    r = rows(4)
    y[r] = -y[r]
    y[rows(5)] = 0.5 * (A[:, 0] + A[:, -1])
    r = rows(6)
    y[r] = y[r] + rng.normal(scale=0.3, size=(len(r), nS))
    y[rows(7)] = 1.0
    y[rows(8)] = A @ np.full(n_atoms, 1.0 / n_atoms)
    r = rows(9)
    y[r] = A[:, rng.integers(n_atoms, size=len(r))].T * (1.0 + 2.0 ** -40)
    if not exact:
        r = np.flatnonzero((v % 3 == 0) & np.isin(kind, (1, 8, 9)))
        y[r] = np.abs(y[r] + rng.normal(scale=0.02, size=(len(r), nS)))
    y[v % 5 == 1] *= UP
    y[v % 5 == 3] *= DOWN
    return np.ascontiguousarray(y), kind


def easy_signals(A, n, rng, snr=20.0):
    """well-posed voxels of the dictionary A: a Dirichlet mixture of three random atoms, Rician noise"""
    A = np.asarray(A, dtype=np.float64)
    w = rng.dirichlet([2.0, 2.0, 1.0], n)
    k = rng.integers(A.shape[1], size=(n, 3))
    y0 = sum(w[:, c:c + 1] * A[:, k[:, c]].T for c in range(3))
    s = 1.0 / snr
    return np.abs(y0 + rng.normal(scale=s, size=y0.shape) + 1j * rng.normal(scale=s, size=y0.shape))


# ------------------------------------------------------------------------------------------------ certificate
def gradient(A, y, x, lam1, lam2):
    """g = A'(y - A x) - lambda2 x - lambda1 of every voxel, float64 from a long-double residual (czb_np.czb_gradient for voxels
    of one dictionary; x are the coefficients the solver works with: SANDI's before the rescaling by the norms)"""
    Al = np.asarray(A, dtype=np.float64).astype(LD)
    X = np.asarray(x, dtype=np.float64).astype(LD)
    res = np.asarray(y, dtype=np.float64).astype(LD) - X @ Al.T
    return (res @ Al - LD(lam2) * X - LD(lam1)).astype(np.float64)


def certificate(A, y, x, lam1, lam2):
    """per voxel (max |g_P|, max g_Z, min x): the Kuhn-Tucker conditions of min 1/2 |y - A x|^2 + lambda1 sum x + lambda2 / 2 |x|^2,
    x >= 0 -- zero on the passive atoms (x > 0), <= 0 on the clamped ones.  Empty sets give 0."""
    g = gradient(A, y, x, lam1, lam2)
    P = np.asarray(x) > 0
    gp = np.where(P, np.abs(g), 0.0).max(axis=1)
    gz = np.where(P, -np.inf, g).max(axis=1)
    gz = np.where(np.isfinite(gz), np.maximum(gz, 0.0), 0.0)
    return gp, gz, np.asarray(x).min(axis=1)


# ------------------------------------------------------------------------------------------------ maps
def _seq_sum(x, cols):
    """the columns of x added one after the other, as the reference's loops do"""
    s = np.zeros(x.shape[0])
    for j in cols:
        s = s + x[:, j]
    return s


def fw_maps(x, n_perp, is_mouse):
    """models.pyx:1240-1256: v, 1 - v (+ v_blood, v_csf for Mouse) from the coefficients x [n, n_atoms]"""
    x = np.asarray(x, dtype=np.float64)
    x_sum = _seq_sum(x, range(x.shape[1])) + 1e-16
    v = _seq_sum(x, range(n_perp)) / x_sum
    cols = [v, 1.0 - v]
    if is_mouse:
        cols += [x[:, n_perp] / x_sum, x[:, n_perp + 1] / x_sum]
    return np.stack(cols, axis=1)


def sandi_maps(x, n_rs, n_in, Rs, d_in, d_isos):
    """models.pyx:1573-1612: fsoma, fneurite, fextra, Rsoma [um], Din, De [um^2/ms] from the RESCALED coefficients x [n, n_atoms]
    (x * norms, models.pyx:1570-1571), the 1e-16 guards in the reference's order"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    sph, stk, iso = range(n_rs), range(n_rs, n_rs + n_in), range(n_rs + n_in, n)
    x_sum = _seq_sum(x, range(n)) + 1e-16
    xsph, xstk, xiso = _seq_sum(x, sph), _seq_sum(x, stk), _seq_sum(x, iso)
    f = [xsph / x_sum, xstk / x_sum, xiso / x_sum]

    def moment(cols, w):
        s = np.zeros(x.shape[0])
        for k, j in enumerate(cols):
            s = s + float(w[k]) * x[:, j]
        return s
    Rsoma, Din, De = moment(sph, Rs), moment(stk, d_in), moment(iso, d_isos)
    return np.stack(f + [1e6 * Rsoma / (xsph + 1e-16), 1e3 * Din / (xstk + 1e-16), 1e3 * De / (xiso + 1e-16)], axis=1)


# ------------------------------------------------------------------------------------------------ error maps
def _residual_sq(A, y, x):
    Al = np.asarray(A, dtype=np.float64).astype(LD)
    r = np.asarray(y, dtype=np.float64).astype(LD) - np.asarray(x, dtype=np.float64).astype(LD) @ Al.T
    return (r * r).sum(axis=1)


def rmse_ld(A, y, x):
    """sqrt(mean (y - A x)^2) per voxel from a long-double residual.  SANDI: pass the RESCALED x with the NORMALISED A -- the quirk
    of models.pyx:1571 / 1615, which the oracle and the device keep"""
    return np.sqrt(_residual_sq(A, y, x) / LD(np.asarray(y).shape[1])).astype(np.float64)


def nrmse_ld(A, y, x):
    """sqrt(sum (y - A x)^2 / sum y^2) where sum y^2 > 1e-16, else 0 (the reference's guard)"""
    ysq = (np.asarray(y, dtype=np.float64).astype(LD) ** 2).sum(axis=1)
    ok = ysq > LD(1e-16)
    out = np.zeros(len(ysq), dtype=LD)
    out[ok] = np.sqrt(_residual_sq(A, y, x)[ok] / ysq[ok])
    return out.astype(np.float64)


def fw_corrected(y, x_iso, csf):
    """models.pyx:1264-1274: y minus the isotropic part, clipped at 0 (csf [n_iso, nS] float64, x_iso [n, n_iso])"""
    yc = np.asarray(y, dtype=np.float64) - np.asarray(x_iso, dtype=np.float64) @ np.asarray(csf, dtype=np.float64)
    return np.where(yc < 0, 0.0, yc)


# ------------------------------------------------------------------------------------------------ dictionaries
FW_ORI = np.array([17, 203, 431])           # three LUT orientations ...
FW_COUNTS = (2100, 835, 65)                 # ... three units of the fused kernel + ring wrap + ragged tile | one unit | one tile + 1 voxel
FW_D_PERPS = {10: None, 14: np.linspace(0.05, 1.0, 14) * 1e-3, 19: np.linspace(0.05, 1.0, 19) * 1e-3}
SANDI_ATOMS = {12: (4, 4, 4), 15: (5, 5, 5), 16: (6, 5, 5), 20: (7, 7, 6)}
# number of volumes -> (b0 volumes, directions on each of the five shells) of the protocols without a directional average
SANDI_SCHEMES = {100: dict(ndir_per_shell=19, n_b0=5), 128: dict(ndir_per_shell=24, n_b0=8), 129: dict(ndir_per_shell=24, n_b0=9)}


@functools.lru_cache(maxsize=None)
def _htable():
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'htable500.npz'), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def fw_dictionary(n_dwi, n_perp=10, mouse=False):
    """(scheme, K): 1 b0 + n_dwi volumes at b = 1000, n_perp zeppelins (the reference's ten, or 14 / 19 over the same range), one
    isotropic atom, two for Mouse -- S.freewater_kernels on the 500 LUT orientations"""
    from amico_amd import synthetic as S
    sch = S.make_scheme(1, ((1000.0, n_dwi),), seed=3)
    K = S.freewater_kernels(sch, _htable()['dirs'], d_perps=FW_D_PERPS[n_perp], d_isos=(1.5e-3, 3e-3) if mouse else (2.5e-3,))
    return sch, K


def fw_matrix(K, lid):
    """A [nS, n_atoms] float64 of LUT orientation lid: zeppelins | isotropic (models.pyx:1233-1235)"""
    return np.concatenate([K['D'][:, lid, :], K['CSF']], axis=0).astype(np.float64).T


@functools.lru_cache(maxsize=None)
def sandi_dictionary(nS=6, n_atoms=15):
    """(scheme, K, Rs, d_in, d_isos).  nS = 6: the default protocol after the directional average; 4: three shells averaged; 100 /
    128 / 129: five shells without the average.  n_atoms 15: the model's defaults, otherwise the same ranges resampled"""
    from amico_amd import synthetic as S
    if nS == 6:
        sch = S.directional_average_scheme(S.make_sandi_scheme())
    elif nS == 4:
        sch = S.directional_average_scheme(S.make_sandi_scheme(bvals=(1000., 4000., 8000.)))
    else:
        sch = S.make_sandi_scheme(**SANDI_SCHEMES[nS])
    assert sch.nS == nS
    a, b, c = SANDI_ATOMS[n_atoms]
    if n_atoms == 15:
        K, Rs, d_in, d_isos = S.sandi_kernels(sch)
    else:
        K, Rs, d_in, d_isos = S.sandi_kernels(sch, Rs=np.linspace(1.0, 12.0, a) * 1e-6, d_in=np.linspace(0.25, 3.0, b) * 1e-3,
                                              d_isos=np.linspace(0.25, 3.0, c) * 1e-3)
    return sch, K, Rs, d_in, d_isos


def sandi_matrix(K):
    """A [nS, n_atoms] float64, columns normalised: what the solver works with (models.pyx:1569)"""
    return np.ascontiguousarray(K['signal'], dtype=np.float64)


def fw_problem(K, counts=FW_COUNTS, seed=0, f32=False):
    """hard_mix voxels of FW_ORI with counts voxels each, the orientations interleaved in memory as a brain's are:
    (y [n, nS], dirs [n, 3], lut [n], kind [n]).  f32: the samples rounded to float32 (and widened again)"""
    h = _htable()
    rng = np.random.default_rng(seed)
    lut = rng.permutation(np.repeat(FW_ORI[:len(counts)], counts))
    d = Z.dirs_in_cells(lut, h['dirs'], h['htable'], rng)
    y = np.zeros((len(lut), K['CSF'].shape[1]))
    kind = np.zeros(len(lut), dtype=np.int64)
    for k, lid in enumerate(FW_ORI[:len(counts)]):
        rows = np.flatnonzero(lut == lid)
        A = fw_matrix(K, lid)
        y[rows], kind[rows] = hard_mix(A, easy_signals(A, len(rows), rng), seed * 7 + k)
    if f32:
        y = y.astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(y), d, lut, kind


def sandi_problem(K, n=3000, seed=0, f32=False, exact=True):
    """(y [n, nS], kind [n]): hard_mix on mixtures of the normalised atoms"""
    A = sandi_matrix(K)
    rng = np.random.default_rng(seed)
    y, kind = hard_mix(A, easy_signals(A, n, rng, snr=50.0), seed, exact=exact)
    if f32:
        y = y.astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(y), kind


# ------------------------------------------------------------------------------------------------ the standard, shared by both tests
KKT = 1e-9            # the project's W_P_TOL / W_Z_TOL (test_gpu_kkt.py), per voxel and relative to s = max |y| of the voxel


def scale_of(y):
    return np.abs(np.asarray(y)).max(axis=1)


def kkt_ok(A, y, x, lam1, lam2):
    """the certificate the GPU test holds every voxel to, per voxel (ok [n], gP / s, gZ / s): min x >= 0, max |g_P| < 1e-9 s and
    max g_Z < 1e-9 s with s = max |y| of the voxel; an all-zero voxel (s = 0) must have x exactly 0"""
    gp, gz, mn = certificate(A, y, x, lam1, lam2)
    s = scale_of(y)
    zero = s == 0
    sc = np.where(zero, 1.0, s)
    ok = np.where(zero, (np.asarray(x) == 0).all(axis=1), (mn >= 0) & (gp < KKT * s) & (gz < KKT * s))
    return ok, gp / sc, gz / sc


def degenerate(xo, go, bound):
    """atoms that may sit on either side of the support: oracle coefficient (passive) or dual value (clamped) within bound [n] of 0
    -- the rule of test_gpu_czb_paths.py, per voxel"""
    b = np.asarray(bound)[:, None]
    return np.where(xo > 0, xo <= b, np.abs(go) <= b)


# ------------------------------------------------------------------------------------------------ the route table
def _case(route, lams, **kw):
    d = dict(route=route, lams=tuple(lams), n_perp=10, mouse=False, f32=False, env={}, rmse=False, nrmse=False, corrected=False, n_atoms=15, exact=True)
    d.update(kw)
    return d


FW_DEFAULT, SANDI_DEFAULT = (0.0, 1e-3), (0.0, 5e-3)
WAVE = {'AMX_WAVE_PER_VOXEL': '1'}
FUSED11, FUSED12 = 'k_freewater_fused<11>', 'k_freewater_fused<12>'
REFILL_MFMA, REFILL_VALU = 'k_fw_project_mfma -> k_freewater_refill', 'k_fw_project -> k_freewater_refill'
FW_LANE, FW_WAVE = 'k_freewater_lane', 'k_freewater (wavefront per voxel)'
# FreeWater: 1 b0 + n_dwi volumes.  (The wavefront-per-voxel kernel holds 2 / 4 / 8 signal rows per lane up to 128 / 256 / 512 volumes.)
FW_CASES = {
    'fused11': _case(FUSED11, [FW_DEFAULT], n_dwi=64),                                   # tail nS & 15 = 1
    'fused11_lam1': _case(FUSED11, [(0.05, 2e-2)], n_dwi=63),                            # the lower edge, nS = 64
    'fused12_f32': _case(FUSED12, [FW_DEFAULT], n_dwi=95, mouse=True, f32=True),         # the upper edge, nS = 96
    'refill_mfma': _case(REFILL_MFMA, [FW_DEFAULT], n_dwi=32),
    'refill_nofuse12': _case(REFILL_MFMA, [FW_DEFAULT], n_dwi=64, mouse=True, env={'AMX_FW_NO_FUSE': '1'}),
    'refill_valu': _case(REFILL_VALU, [FW_DEFAULT], n_dwi=129),
    'lane11_err': _case(FW_LANE, [FW_DEFAULT], n_dwi=64, rmse=True, nrmse=True, corrected=True),
    'lane12_err': _case(FW_LANE, [FW_DEFAULT], n_dwi=64, mouse=True, rmse=True),
    'lane16': _case(FW_LANE, [FW_DEFAULT], n_dwi=64, n_perp=14, mouse=True),
    'lane_long': _case(FW_LANE, [FW_DEFAULT], n_dwi=240),                                # beyond the refill kernel's LDS bound
    'lane_cold': _case(FW_LANE, [(0.0, 1e-6)], n_dwi=64),                                # below amx_warm_start: Lawson-Hanson loop
    'lane_edge': _case(FW_LANE, [(0.0, 1e-9)], n_dwi=64),                                # the weakest ridge a lane takes
    'wave_qr': _case(FW_WAVE, [(0.0, 5e-10), (0.0, 0.0)], n_dwi=64),
    'wave20': _case(FW_WAVE, [FW_DEFAULT], n_dwi=64, n_perp=19),
    'wave4': _case(FW_WAVE, [FW_DEFAULT], n_dwi=129, env=WAVE),
    'wave8': _case(FW_WAVE, [FW_DEFAULT], n_dwi=299, env=WAVE),
}
ROWS, S_LANE, S_WAVE = 'k_sandi_rows<6,15>', 'k_sandi_lane', 'k_sandi (wavefront per voxel)'
# SANDI: nS volumes (6 and 4: after the directional average), n_atoms
SANDI_CASES = {
    'rows': _case(ROWS, [SANDI_DEFAULT, (0.01, 5e-2)], nS=6, rmse=True),
    'lane15': _case(S_LANE, [SANDI_DEFAULT], nS=6, env={'AMX_SANDI_ATOM_SPACE': '1'}, rmse=True, nrmse=True),
    'lane15_cold': _case(S_LANE, [(0.0, 2e-6)], nS=6),
    'lane15_edge': _case(S_LANE, [(0.0, 1e-9)], nS=6, exact=False),
    'lane12': _case(S_LANE, [SANDI_DEFAULT], nS=6, n_atoms=12),
    'lane16': _case(S_LANE, [SANDI_DEFAULT], nS=6, n_atoms=16),
    'lane_rows4': _case(S_LANE, [SANDI_DEFAULT], nS=4),                                  # not the 6 x 15 tables
    'lane_128': _case(S_LANE, [SANDI_DEFAULT], nS=128),                                  # kSandiShortNS
    'wave1': _case(S_WAVE, [(0.0, 0.0)], nS=6, exact=False),
    'wave2': _case(S_WAVE, [(0.0, 5e-10)], nS=100, exact=False),
    'wave20': _case(S_WAVE, [SANDI_DEFAULT], nS=6, n_atoms=20),
    'long_lane15': _case('k_sandi_gram_lane<15>', [SANDI_DEFAULT], nS=129),
    'long_lane12': _case('k_sandi_gram_lane<12>', [SANDI_DEFAULT], nS=129, n_atoms=12, f32=True),
    'long_lane16': _case('k_sandi_gram_lane<16>', [SANDI_DEFAULT], nS=129, n_atoms=16),
    'long_wave': _case('k_sandi_gram_wave', [SANDI_DEFAULT], nS=129, env=WAVE),
    'long_wave20': _case('k_sandi_gram_wave', [SANDI_DEFAULT], nS=129, n_atoms=20),
    'long_edge': _case('k_sandi_gram_lane<15>', [(0.0, 1e-9)], nS=129, rmse=True, exact=False),
}


def fw_case_dictionary(c):
    return fw_dictionary(c['n_dwi'], c['n_perp'], c['mouse'])


def sandi_case_dictionary(c):
    return sandi_dictionary(c['nS'], c['n_atoms'])


# ------------------------------------------------------------------------------------------------ the reference
def _nnls_rows(groups, y, n_atoms):
    from oracle import oracle
    x = np.zeros((len(y), n_atoms))
    for rows, A in groups:
        for v in rows:
            x[v], _, mode = oracle.nnls(A, y[v])
            assert mode == 1, (int(v), mode)
    return x


def fw_groups(K, lut):
    """[(rows, A)] per LUT orientation present in lut"""
    return [(np.flatnonzero(lut == lid), fw_matrix(K, lid)) for lid in np.unique(lut)]


def fw_reference(K, c, lam, y, d, lut, nthreads=4):
    """(x, maps) of the CPU oracle.  With lambda2 > 0 that is oracle.freewater_fit.  With lambda1 = lambda2 = 0 the problem is plain
    NNLS and the reference is the oracle's Lawson-Hanson solver in A-space, as in test_czb_without_a_ridge: the oracle's elastic net
    follows the LARS path with a Cholesky factor of the active Gram block, which at cond(A'A) = 4e16 loses positive definiteness
    (status -1, which the model loop ignores) -- on the uniform mixture of FreeWater's atoms it stops half-way along the path, with
    a Kuhn-Tucker residual of 0.07."""
    from oracle import oracle
    if lam[1] == 0.0:
        assert lam[0] == 0.0
        x = _nnls_rows(fw_groups(K, lut), y, K['D'].shape[0] + K['CSF'].shape[0])
        return x, fw_maps(x, c['n_perp'], c['mouse'])
    ref = oracle.freewater_fit(y, d, K, _htable()['htable'], lam[0], lam[1], is_mouse=c['mouse'], nthreads=nthreads, return_x=True)
    assert ref['err'] == 0, ref['err']
    return ref['x'], ref['estimates']


def sandi_reference(K, Rs, d_in, d_isos, lam, y, nthreads=4):
    """(x of the solver -- before the rescaling by the norms --, maps); lambda2 = 0 as fw_reference"""
    from oracle import oracle
    if lam[1] == 0.0:
        assert lam[0] == 0.0
        x = _nnls_rows([(np.arange(len(y)), sandi_matrix(K))], y, len(K['norms']))
        return x, sandi_maps(x * K['norms'][None, :], len(Rs), len(d_in), Rs, d_in, d_isos)
    ref = oracle.sandi_fit(y, K, Rs, d_in, d_isos, lam[0], lam[1], nthreads=nthreads, return_x=True)
    return ref['x'] / K['norms'][None, :], ref['estimates']


def map_distance(maps, ref):
    """per voxel: fractions absolute, SANDI's sizes (columns 3 ..) as |d| / (|ref| + 1e-3) -- test_sandi_kkt_certificates"""
    d = np.abs(maps - ref)
    if maps.shape[1] == 6:
        d[:, 3:] = d[:, 3:] / (np.abs(ref[:, 3:]) + 1e-3)
    return d.max(axis=1)
