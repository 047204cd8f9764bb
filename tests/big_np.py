"""FreeWater, SANDI and CylinderZeppelinBall on dictionaries of 65 .. 256 atoms: the shapes, signals and CPU references that
test_big_dictionaries.py (the oracle alone) and test_gpu_big_dictionaries.py (the device route k_enet_big) share.  The signals are
small_np.hard_mix on every dictionary -- all-zero, one-atom, isotropic-only, pure-noise, negated ... voxels, amplitudes 2^-20, 1 and
2^20 side by side -- 365 voxels over three LUT orientations with unequal counts.  CPU only; nothing here touches the library under test.

The shapes are the smallest at which the route can go wrong: 65 atoms (the first past the cap of the wavefront-per-voxel kernels, across
the 64-lane and 64-bit-mask boundaries), 101 (no multiple of 16), 256 (the bound: every thread an atom), more atoms than samples
(21 x 256; SANDI 6 x 65, 6 x 256: the rank guard), the largest tile 512 x 256 once on 64 voxels, SANDI on both sides of 128 volumes at
90 atoms, Mouse FreeWater at 65 atoms, and a 64-atom dictionary of each model, which must take none of the new kernels.  With
lambda1 = lambda2 = 0 the reference is the oracle's A-space NNLS (small_np.fw_reference / sandi_reference)."""
import functools
import zlib

import numpy as np

import czb_np as Z
import small_np as N

ORI = N.FW_ORI                         # three LUT orientations of the 500
COUNTS = (230, 100, 35)                # 365 voxels, unequal
COUNTS_TILE = (40, 20, 4)              # the 512 x 256 tile: 64 voxels
D_PAR = 0.6e-3                         # CylinderZeppelinBall (test_gpu_czb_paths.py)
CZB_DEFAULT = (0.0, 4.0)


def _case(model, lams, **kw):
    d = dict(model=model, lams=tuple(lams), counts=COUNTS, mouse=False, f32=False, exact=True, small=False)
    d.update(kw)
    return d


# FreeWater: nS volumes (1 b0 + nS - 1 at b = 1000), n_perp zeppelins + 1 isotropic atom (2 for Mouse)
# SANDI: nS volumes (6: after the directional average; 100 / 129: five shells without it), atoms = (radii, d_in, d_isos)
# CylinderZeppelinBall: nS volumes, n_atoms = radii + 4 zeppelins + 1 ball (czb_np.atom_sets)
CASES = {
    'fw_33x65': _case('fw', [N.FW_DEFAULT, (0.05, 2e-2)], nS=33, n_perp=64),
    'fw_33x101': _case('fw', [N.FW_DEFAULT], nS=33, n_perp=100),
    'fw_21x256': _case('fw', [N.FW_DEFAULT, (0.0, 0.0)], nS=21, n_perp=255),
    'fw_mouse_33x65': _case('fw', [N.FW_DEFAULT], nS=33, n_perp=63, mouse=True, f32=True),
    'fw_512x256': _case('fw', [N.FW_DEFAULT], nS=512, n_perp=255, counts=COUNTS_TILE),
    'fw_33x64': _case('fw', [N.FW_DEFAULT], nS=33, n_perp=63, small=True),
    'sandi_6x65': _case('sandi', [N.SANDI_DEFAULT], nS=6, atoms=(22, 22, 21)),
    'sandi_6x256': _case('sandi', [N.SANDI_DEFAULT, (0.01, 5e-2)], nS=6, atoms=(86, 85, 85)),
    'sandi_100x90': _case('sandi', [N.SANDI_DEFAULT], nS=100, atoms=(30, 30, 30)),
    'sandi_129x90': _case('sandi', [N.SANDI_DEFAULT], nS=129, atoms=(30, 30, 30), f32=True),
    'sandi_100x65': _case('sandi', [(0.0, 0.0)], nS=100, atoms=(22, 22, 21), exact=False),
    'sandi_6x64': _case('sandi', [N.SANDI_DEFAULT], nS=6, atoms=(22, 21, 21), small=True),
    'czb_40x65': _case('czb', [CZB_DEFAULT], nS=40, n_atoms=65),
    'czb_40x130': _case('czb', [CZB_DEFAULT, (0.0, 1e-3)], nS=40, n_atoms=130),
    'czb_33x256': _case('czb', [CZB_DEFAULT], nS=33, n_atoms=256),
    'czb_40x64': _case('czb', [CZB_DEFAULT], nS=40, n_atoms=64, small=True),
}
RUNS = [(name, lam) for name, c in CASES.items() for lam in c['lams']]
BIG_RUNS = [(name, lam) for name, lam in RUNS if not CASES[name]['small']]
SMALL_RUNS = [(name, lam) for name, lam in RUNS if CASES[name]['small']]
NEW_KERNEL = 'k_enet_big'


def ids(runs):
    return ['%s-%g-%g' % (n, l[0], l[1]) for n, l in runs]


def seed_of(name):
    return zlib.crc32(name.encode()) % 10_000


def n_atoms_of(c):
    if c['model'] == 'fw':
        return c['n_perp'] + (2 if c['mouse'] else 1)
    return sum(c['atoms']) if c['model'] == 'sandi' else c['n_atoms']


# ------------------------------------------------------------------------------------------------ dictionaries
@functools.lru_cache(maxsize=None)
def dictionary(name):
    """FreeWater: (K,); SANDI: (K, Rs, d_in, d_isos); CylinderZeppelinBall: (K, Rs, n_perp)"""
    from amico_amd import synthetic as S
    c = CASES[name]
    h = N._htable()
    if c['model'] == 'fw':
        sch = S.make_scheme(1, ((1000.0, c['nS'] - 1),), seed=3)
        K = S.freewater_kernels(sch, h['dirs'], d_perps=np.linspace(0.05, 1.0, c['n_perp']) * 1e-3, d_isos=(1.5e-3, 3e-3) if c['mouse'] else (2.5e-3,))
        assert K['D'].shape == (c['n_perp'], 500, c['nS'])
        return (K,)
    if c['model'] == 'sandi':
        sch = S.directional_average_scheme(S.make_sandi_scheme()) if c['nS'] == 6 else S.make_sandi_scheme(**N.SANDI_SCHEMES[c['nS']])
        assert sch.nS == c['nS']
        a, b, cc = c['atoms']
        return S.sandi_kernels(sch, Rs=np.linspace(1.0, 12.0, a) * 1e-6, d_in=np.linspace(0.25, 3.0, b) * 1e-3, d_isos=np.linspace(0.25, 3.0, cc) * 1e-3)
    Rs, d_perps, d_isos = Z.atom_sets(c['n_atoms'])
    K = Z.czb_kernels(Z.make_scheme(c['nS'], seed=c['nS']), ORI, Rs, d_perps, d_isos, D_PAR, lut_dirs=h['dirs'])
    return K, Rs, len(d_perps)


def matrix(name, lid):
    """A [nS, n_atoms] float64 of LUT orientation lid (SANDI: the one dictionary, columns normalised)"""
    c, D = CASES[name], dictionary(name)
    if c['model'] == 'fw':
        return N.fw_matrix(D[0], lid)
    return N.sandi_matrix(D[0]) if c['model'] == 'sandi' else Z.dictionary(D[0], lid)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(y [n, nS], dirs [n, 3] or None, lut [n], kind [n]), read-only: hard_mix voxels, the orientations interleaved in memory"""
    c = CASES[name]
    h = N._htable()
    seed = seed_of(name)
    rng = np.random.default_rng(seed)
    n = sum(c['counts'])
    if c['model'] == 'sandi':
        A = matrix(name, 0)
        y, kind = N.hard_mix(A, N.easy_signals(A, n, rng, snr=50.0), seed, exact=c['exact'])
        d, lut = None, np.zeros(n, dtype=np.int64)
    else:
        lut = rng.permutation(np.repeat(ORI, c['counts']))
        d = Z.dirs_in_cells(lut, h['dirs'], h['htable'], rng)
        y, kind = np.zeros((n, c['nS'])), np.zeros(n, dtype=np.int64)
        for k, lid in enumerate(ORI):
            rows = np.flatnonzero(lut == lid)
            A = matrix(name, lid)
            y[rows], kind[rows] = N.hard_mix(A, N.easy_signals(A, len(rows), rng), seed * 7 + k)
    if c['f32']:
        y = y.astype(np.float32).astype(np.float64)
    y = np.ascontiguousarray(y)
    for a in (y, d, lut, kind):
        if a is not None:
            a.setflags(write=False)
    return y, d, lut, kind


def groups(name):
    """[(rows, A)] per dictionary present"""
    _, _, lut, _ = problem(name)
    return [(np.flatnonzero(lut == lid), matrix(name, lid)) for lid in np.unique(lut)]


def solver_x(name, x):
    """the coefficients the solver works with, from what the device / the maps hold (SANDI: before the rescaling by the norms)"""
    return x / dictionary(name)[0]['norms'][None, :] if CASES[name]['model'] == 'sandi' else x


def maps_of(name, x):
    """the model's maps from the solver's coefficients x [n, n_atoms] (models.pyx:1240-1256 / 1570-1612 / 616-633)"""
    c, D = CASES[name], dictionary(name)
    if c['model'] == 'fw':
        return N.fw_maps(x, c['n_perp'], c['mouse'])
    if c['model'] == 'sandi':
        K, Rs, d_in, d_isos = D
        return N.sandi_maps(x * K['norms'][None, :], len(Rs), len(d_in), Rs, d_in, d_isos)
    return Z.czb_maps(x, D[1], D[2])


@functools.lru_cache(maxsize=None)
def reference(name, lam, nthreads=4):
    """(x of the solver, maps) of the CPU oracle, read-only; lambda1 = lambda2 = 0: the oracle's Lawson-Hanson NNLS in A-space"""
    from oracle import oracle
    c, D = CASES[name], dictionary(name)
    y, d, lut, _ = problem(name)
    ht = N._htable()['htable']
    if c['model'] == 'fw':
        x, m = N.fw_reference(D[0], c, lam, y, d, lut, nthreads=nthreads)
    elif c['model'] == 'sandi':
        x, m = N.sandi_reference(D[0], D[1], D[2], D[3], lam, y, nthreads=nthreads)
    elif lam[1] == 0.0:
        x = N._nnls_rows(groups(name), y, n_atoms_of(c))
        m = maps_of(name, x)
    else:
        ref = oracle.czb_fit(y, d, D[0], D[1], ht, lam[0], lam[1], nthreads=nthreads, return_x=True)
        assert ref['err'] == 0, ref['err']
        x, m = ref['x'], ref['estimates']
    x.setflags(write=False); m.setflags(write=False)
    return x, m


def certificate(name, x, lam):
    """small_np.kkt_ok of the solver's coefficients x on every voxel: (ok [n], gP / s [n], gZ / s [n])"""
    y = problem(name)[0]
    n = len(y)
    ok, gp, gz = np.zeros(n, bool), np.zeros(n), np.zeros(n)
    for rows, A in groups(name):
        ok[rows], gp[rows], gz[rows] = N.kkt_ok(A, y[rows], x[rows], lam[0], lam[1])
    return ok, gp, gz


# ------------------------------------------------------------------------------------------------ the pivot of a nearly dependent atom
def pivots_of_last_atom(A, P, lam2=0.0):
    """the Cholesky pivot of the last atom of P (a list of columns of A) behind the others, three ways: (Gram space in float64: H_jj - |l|^2
    with L l = H_Pj; A-space in float64, as k_enet_big evaluates a small pivot: |a_j - A_P w|^2 + lambda2 (1 + |w|^2) with L'w = l; the
    same in long double from a long-double factor) -- each divided by H_jj -- and the floor below which k_enet_big takes the A-space value for
    noise: (32 eps)^2 (1 + |w|_1)^2 / rho, rho the smallest pivot ratio L_ss^2 / H_ss of the atoms before"""
    A = np.asarray(A, dtype=np.float64)
    P, j = list(P[:-1]), P[-1]
    H = A[:, P].T @ A[:, P] + lam2 * np.eye(len(P))
    hj = A[:, j] @ A[:, j] + lam2
    L = np.linalg.cholesky(H)
    ell = np.linalg.solve(L, A[:, P].T @ A[:, j])
    gram = hj - ell @ ell
    w = np.linalg.solve(L.T, ell)
    d = A[:, j] - A[:, P] @ w
    aspace = d @ d + lam2 * (1.0 + w @ w)
    Al = A.astype(N.LD)
    Hl = Al[:, P].T @ Al[:, P] + N.LD(lam2) * np.eye(len(P), dtype=N.LD)
    wl = w.astype(N.LD)
    for _ in range(4):                                    # (refined in long double against the long-double normal equations)
        wl = wl + np.linalg.solve(H, (Al[:, P].T @ Al[:, j] - Hl @ wl).astype(np.float64)).astype(N.LD)
    dl = Al[:, j] - Al[:, P] @ wl
    exact = dl @ dl + N.LD(lam2) * (1 + wl @ wl)
    rho = float((np.diag(L) ** 2 / np.diag(H)).min())
    floor = 1024 * np.finfo(np.float64).eps ** 2 * (1.0 + np.abs(w).sum()) ** 2 / rho      # (amx_bpp.hpp: kFloor)
    return float(gram / hj), float(aspace / hj), float(exact / N.LD(hj)), floor
