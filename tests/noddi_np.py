"""NODDI in plain numpy, for the hard-voxel tests of the seeded chain at every shape edge (test_noddi_hard.py, test_gpu_noddi_hard.py):
the case table, the signals, the CPU reference, the maps of models.pyx:945-967 restated from the stage-3 coefficients, the error maps
from long-double residuals.  CPU only; the only thing asked of the library under test is the arithmetic of its route (_capi.noddi_route,
no device), to find the shapes at which a route changes.  The per-voxel certificate is kkt_certificates.noddi_certificates_per_voxel."""
import functools
import os
import zlib

import numpy as np

import czb_np as Z
from kkt_certificates import by_direction, noddi_certificates_per_voxel
from small_np import _htable, degenerate      # noqa: F401  (degenerate: the rule of test_gpu_czb_paths.py, shared)

LD = np.longdouble
NTHREADS = min(16, os.cpu_count() or 1)

# ------------------------------------------------------------------------------------------------ the standard
KKT = 1e-9            # the project's W_P_TOL / W_Z_TOL, per voxel and relative to s = max|y| of the voxel
ORACLE_KKT = 1e-11    # what the oracle's own x must meet on the same signals (measured: <= 2e-13)
DEGENERATE = 1e-7     # times s: a stage-2 coefficient or the dual value of a clamped atom this close to zero may sit on either side
XISO_TOL = 1e-7       # times s: x_iso handed from stage 1 to stage 2, against the oracle's
AX_TOL = 1e-4         # times s: A2 x against the oracle's where czb_np.x_bound exceeds 1e-6
MAP_TOL = 1e-6
MAX_SHARE = 0.01      # of a case's voxels: degenerate for the oracle / excused from the oracle comparison of the maps

# ------------------------------------------------------------------------------------------------ signals
ORI = np.array([17, 203, 431])       # the three LUT orientations that occur ...
COUNTS = (2100, 835, 65)             # ... with AMX_SEED_CHUNK=256: nine seed chunks with a ragged last one | four | a quarter of one
AMPS = (2.0 ** -8, 1.0, 2.0 ** 6)    # voxel v is scaled by AMPS[v % 3]: lambda1 is absolute, so these are three different problems
N_SMALL = sum(COUNTS)
_N_DRAW = 4000
_CELL_SHARES = (0.65, 0.97)          # of the sphere's cells that draw orientation 0 | 1 | 2: every population is reached within _N_DRAW voxels


def hard_signals(K, sch, seed):
    """(y [3000, nS] float32 values in float64, dirs [3000, 3], kind, amp index): synthetic.noddi_hard_signals on the dictionary K --
    crossings, the minor fibre's direction, pure noise, flat, half zeroed, CSF dominated, background, SNR 5 / 15 / 40, the first ten
    voxels all zero -- drawn on a sphere whose cells name one of the three orientations ORI only, then the first 2 100 / 835 / 65 voxels
    of each orientation kept in the order they were drawn (interleaved in memory, as a brain's voxels are) and every direction replaced
    by one inside the true LUT cell of its orientation."""
    from amico_amd import synthetic as S
    h = _htable()
    rng = np.random.default_rng(seed)
    cells = np.searchsorted(_CELL_SHARES, rng.random(181 * 181)).astype(np.int16)
    sub = {'wm': np.ascontiguousarray(K['wm'][:, ORI, :]), 'iso': K['iso']}
    y, dd, kind = S.noddi_hard_signals(_N_DRAW, sub, cells, sch, seed=seed)
    grp = S.lut_indices(dd, cells)
    keep = np.zeros(_N_DRAW, dtype=bool)
    for g, c in enumerate(COUNTS):
        idx = np.flatnonzero(grp == g)
        assert len(idx) >= c, (g, len(idx))
        keep[idx[:c]] = True
    assert keep[:10].all()
    y, kind, grp = y[keep], kind[keep], grp[keep]
    d = Z.dirs_in_cells(ORI[grp], h['dirs'], h['htable'], rng)
    amp = np.arange(len(y)) % 3
    y = (y * np.asarray(AMPS)[amp][:, None]).astype(np.float32).astype(np.float64)
    assert not y[:10].any() and len(y) == N_SMALL
    return np.ascontiguousarray(y), d, kind, amp


def with_bad_voxels(y, d):
    """two more voxels behind the others: copies of voxels 11 and 12 with a NaN sample / +Inf in the last sample"""
    bad = np.array(y[[11, 12]])
    bad[0, 3] = np.nan
    bad[1, -1] = np.inf
    return np.ascontiguousarray(np.vstack([y, bad])), np.ascontiguousarray(np.vstack([d, d[[11, 12]]]))


def tiled(a, n):
    """a [m, ...] repeated to n rows, every period rotated by one more row: a copy of a voxel lands in another lane and chunk"""
    m = len(a)
    k = np.arange(n)
    return np.ascontiguousarray(a[(k % m + k // m) % m])


def scale_of(y):
    return np.abs(np.asarray(y)).max(axis=1)


# ------------------------------------------------------------------------------------------------ maps
def noddi_maps(x3, K, exvivo=False):
    """NDI, ODI, FWF (+ the ex-vivo dot fraction) from the stage-3 coefficients x3 [n, n_atoms] (white-matter atoms | dot | iso), as
    models.pyx:945-967 forms them: S = sum of all coefficients + 1e-16; W = sum over the white-matter atoms of x_j / S, + 1e-16;
    f1, f2, k1 = sums of icvf_j, float32(1 - icvf_j), kappa_j times x_j / S / W; NDI = f1 / (f1 + f2 + 1e-16), ODI = 2 / pi atan2(1, k1),
    FWF = x_iso / S, dot = x_dot / S.  Sums run over the atoms in order, one after the other."""
    x = np.asarray(x3, dtype=np.float64)
    n_wm = len(K['icvf'])
    icvf = K['icvf'].astype(np.float64)
    ecvf = (1.0 - icvf).astype(np.float32).astype(np.float64)
    kappa = K['kappa'].astype(np.float64)
    S = np.zeros(len(x))
    for j in range(x.shape[1]):
        S = S + x[:, j]
    S = S + 1e-16
    W = np.zeros(len(x))
    for j in range(n_wm):
        W = W + x[:, j] / S
    W = W + 1e-16
    f1, f2, k1 = np.zeros(len(x)), np.zeros(len(x)), np.zeros(len(x))
    for j in range(n_wm):
        f1 = f1 + icvf[j] * x[:, j] / S / W
        f2 = f2 + ecvf[j] * x[:, j] / S / W
        k1 = k1 + kappa[j] * x[:, j] / S / W
    cols = [f1 / (f1 + f2 + 1e-16), 2.0 / np.pi * np.arctan2(1.0, k1), x[:, -1] / S]
    if exvivo:
        cols.append(x[:, -2] / S)
    return np.stack(cols, axis=1)


def groups_of(K, d, exvivo):
    """[(rows, A [nS, n_atoms] float64)] per LUT orientation: white-matter atoms | dot (ex vivo: ones, models.pyx:843-844) | iso"""
    from amico_amd import synthetic as S
    lut = S.lut_indices(d, _htable()['htable'])
    iso = K['iso'].astype(np.float64)
    fixed = ([np.ones_like(iso)] if exvivo else []) + [iso]
    return [(rows, np.concatenate([K['wm'][:, lut[rows[0]], :].astype(np.float64)] + [f[None, :] for f in fixed], axis=0).T)
            for rows in by_direction(lut)]


def _residual_sq(A, y, x):
    r = np.asarray(y, dtype=np.float64).astype(LD) - np.asarray(x, dtype=np.float64).astype(LD) @ A.astype(LD).T
    return (r * r).sum(axis=1)


def rmse_ld(groups, y, x3):
    """sqrt(mean (y - A x)^2) per voxel from a long-double residual (small_np.rmse_ld per orientation)"""
    out = np.zeros(len(y))
    for rows, A in groups:
        out[rows] = np.sqrt(_residual_sq(A, y[rows], x3[rows]) / LD(y.shape[1])).astype(np.float64)
    return out


def nrmse_ld(groups, y, x3):
    """sqrt(sum (y - A x)^2 / sum y^2) where sum y^2 > 1e-16, else 0 (the reference's guard)"""
    out = np.zeros(len(y))
    for rows, A in groups:
        ysq = (y[rows].astype(LD) ** 2).sum(axis=1)
        ok = ysq > LD(1e-16)
        out[rows[ok]] = np.sqrt(_residual_sq(A, y[rows][ok], x3[rows][ok]) / ysq[ok]).astype(np.float64)
    return out


def stage2_product(K, sch, d, x2, exvivo=False):
    """A2 x2 [n, n_dwi] of every voxel: the column-normalised white-matter atoms on the diffusion-weighted rows (models.pyx:914-926)"""
    n_wm = K['wm'].shape[0]
    dwi = np.asarray(sch.dwi_idx)
    out = np.zeros((len(d), len(dwi)))
    for rows, A in groups_of(K, d, exvivo):
        out[rows] = x2[rows, :n_wm] @ (A[dwi][:, :n_wm] * K['norms'][0][None, :]).T
    return out


# ------------------------------------------------------------------------------------------------ the case table
DEFAULT_LAM = (0.5, 1e-3)
CHAIN = {'AMX_SEED_CHUNK': '256', 'AMX_SEED_MIN_VOXELS': '0'}       # the two switches that make the chain run on 3 000 voxels
BIG_N = 600_000
GEMM_KEYS = {'gemm_n_pass': 'gemm_passes', 'gemm_win': 'gemm_window'}       # the table's names -> the words of _capi.noddi_route


def _protocol(nS, n_b0=9):
    """n_b0 b0 volumes, a third of the rest at b = 700 and two thirds at b = 2000 (the default 9 + 30 + 60 for nS = 99)"""
    n = nS - n_b0
    return n_b0, ((700.0, n // 3), (2000.0, n - n // 3))


P41 = (1, ((700.0, 24), (2000.0, 16)))
P105 = (9, ((700.0, 36), (2000.0, 60)))
P150 = (10, ((700.0, 40), (2000.0, 60), (3000.0, 40)))
LEFT_ALL = ('leftover_stage1', 'leftover_lasso', 'leftover_stage3')
GEMM_25_9, GEMM_25, GEMM_40, GEMM_WIN = 'k_noddi_gemm<false,25,9>', 'k_noddi_gemm<false,25>', 'k_noddi_gemm<false,40>', 'k_noddi_gemm<windows>'
RESCUE, REPAIR, THIRD, BIG = 'k_nnls_gcert<1,rescue>', 'k_nnls_gcert<1,repair>', 'k_lasso_gcert<24,wide,18>', 'k_noddi_lasso_big (supports beyond 64 atoms)'
BIG_ALL, LSEED, WIDE = 'k_noddi_lasso_big (all voxels', 'k_lasso_seed', 'k_lasso_gcert<18,wide>'
SMALL1, SMALL3 = 'k_noddi<1> (left-overs of k_nnls_gcert<1>; small-call build', 'k_noddi<3> (left-overs; small-call build'
F32_8_1, F32_8_3 = 'k_noddi<1> (left-overs of k_nnls_gcert<1>; 8 wavefronts, float32 tile)', 'k_noddi<3> (left-overs; 8 wavefronts, float32 tile)'
PLAIN1, PLAIN3 = 'k_noddi<1> (left-overs of k_nnls_gcert<1>) ->', 'k_noddi<3> (left-overs) ->'
ALL1 = 'k_noddi<1> (all voxels)'


def _case(edge, protocol=None, volumes=None, n_b0=9, grid=(12, 12), exvivo=False, lam=DEFAULT_LAM, env=None, n=N_SMALL, must=(), must_not=(),
          route=None, seeded=True, errors=False, left=(), big_in_path=True, seed=None, signals=None):
    """protocol: (n_b0, shells), or volumes (a count, 'lds_edge' or 'lds_edge+1') with n_b0; grid: (orientation dispersions, volume
    fractions) of the white-matter atoms; env: switches besides CHAIN (large calls: none at all); must / must_not: substrings of
    Context.last_path(); route: the fields of _capi.noddi_route at the defaults (cases without a switch of their own: the route of a call
    of 100 000 voxels, large calls: of n) ; left: the left-over counts of last_seed_stats() that must be non-zero and below n; signals: the
    small case whose 3 000 voxels a large call tiles"""
    return dict(edge=edge, protocol=protocol, volumes=volumes, n_b0=n_b0, grid=grid, exvivo=exvivo, lam=lam, env=dict(env or {}), n=n, must=tuple(must),
                must_not=tuple(must_not), route=route, seeded=seeded, errors=errors, left=tuple(left), big_in_path=big_in_path, seed=seed, signals=signals)


def _rt(gemm, n_pass, win, NR, glob=False, rescue=False, third=False, s1='small', s2='gram_left', s3='small'):
    return {'gemm': gemm, 'gemm_n_pass': n_pass, 'gemm_win': win, 'NR': NR, 'global': glob, 'rescue': rescue, 'third': third, 's1': s1, 's2': s2, 's3': s3}


# What _capi.noddi_route found for the edges that depend on LDS arithmetic (default dictionary of 145 atoms, a call of 100 000 voxels; the
# builds of the stage-1 | stage-3 left-over kernels, the table kernel, its windows, signal rows per lane, global tile, rescue, third pass):
#    90 .. 100 volumes   small | small     K-steps 25 (<false,25,9>), one window
#   101 .. 107           small | small     K-steps 40
#   108, 109 .. 112      f64_nw, f32_nw | small          (two small-call workgroups beside the tile stop fitting a CU: stage 1 first)
#   113, 114, 115 .. 128 f32_nw | f64_nw, f64_nw, f32_nw
#   129 .. 160           f32_8 | f32_8     four rows per lane, rescue pass on
#   161 .. 217           f32_8 | f32_8     two windows
#   218                  f32_nw | f32_8    the last shape with its tile in LDS ('vLDS'): eight wavefronts with 12 passive atoms no longer fit
#   219 .. 256           global            the first global-tile shape ('vGT'): repair, rescue and third pass on
#   257 .. 512           global            eight rows per lane
# (the float32 tile beside one wavefront of the LASSO stage's 64-atom re-run kernel fits a CU's 160 KB up to 218 volumes.)  Windows: 100
# volumes is one window of 100, 161 two windows of 84 (the second holds 77 samples), 512 four windows of 128.
CASES = {
    # ---- dictionary edges, 99 volumes
    'd145': _case('the default dictionary: the baseline', route=_rt('25_9', 1, 100, 2), must=(GEMM_25_9, SMALL1, SMALL3, BIG), must_not=(RESCUE, REPAIR, THIRD),
                  errors=True, left=LEFT_ALL),
    'd146x': _case('ex vivo, 144 + dot + iso', exvivo=True, route=_rt('25_9', 1, 100, 2), must=(GEMM_25_9, SMALL1, BIG), must_not=(RESCUE, THIRD), errors=True,
                   left=LEFT_ALL),
    'd144': _case('13 x 11 = 143 + iso: n_atoms = 9 x 16, iso inside a float32 tile, n_wm odd', grid=(13, 11), route=_rt('25_9', 1, 100, 2),
                  must=(GEMM_25_9, SMALL1, BIG), left=LEFT_ALL),
    'd145x': _case('the same 143 atoms ex vivo: 145 atoms split 143 / 2', grid=(13, 11), exvivo=True, route=_rt('25_9', 1, 100, 2), must=(GEMM_25_9, BIG),
                   left=LEFT_ALL),
    'd101': _case('10 x 10 + iso: six float32 tiles, five straggler atoms', grid=(10, 10), route=_rt('25', 1, 100, 2), must=(GEMM_25 + ' ', BIG), left=LEFT_ALL,
                  seed=4),      # (the name's own seed leaves the largest support at 63 of 100 atoms; this one has two voxels at 66)
    'd13': _case('4 x 3 + iso on 1 b0 + 24 + 16 volumes: no float32 tile at all', grid=(4, 3), protocol=P41, route=_rt('25', 1, 44, 2), must=(GEMM_25 + ' ',),
                 left=('leftover_stage1',)),
    'd64_l0': _case('7 x 9 = 63 atoms at lambda1 = 0: the LASSO seed solver runs, not k_noddi_lasso_big for all', grid=(7, 9), lam=(0.0, 1e-3),
                    route=_rt('25', 1, 100, 2), must=(LSEED, GEMM_25 + ' '), must_not=(BIG_ALL,), left=('leftover_lasso',)),
    'd170': _case('13 x 13 + iso: no basis, every voxel through the stage kernels, tile in LDS', grid=(13, 13), seeded=False,
                  route=_rt('none', 1, 100, 2, s1='f32_nw', s2='gram', s3='f64_nw'), must=(ALL1,), must_not=('k_noddi_gemm', 'seed', 'gcert')),
    'd226': _case('15 x 15 + iso on 41 volumes: four atoms per lane, global tile', grid=(15, 15), protocol=P41, seeded=False,
                  route=_rt('none', 1, 44, 2, glob=True, s1='global', s2='global', s3='global'), must=(ALL1,), must_not=('k_noddi_gemm', 'seed', 'gcert')),
    # ---- protocol edges, default dictionary
    'v100': _case('1 b0 + 99: the single-b0 rule; one window of 100, the last K-steps 25 shape', volumes=100, n_b0=1, route=_rt('25_9', 1, 100, 2),
                  must=(GEMM_25_9, SMALL1), left=LEFT_ALL),
    'v101': _case('the first K-steps 40 shape', volumes=101, route=_rt('40', 1, 104, 2), must=(GEMM_40, SMALL1), left=LEFT_ALL),
    'v128': _case('two signal rows per lane, for the last time', volumes=128, route=_rt('40', 1, 128, 2, s1='f32_nw', s3='f32_nw'), must=(GEMM_40, PLAIN1, PLAIN3), must_not=(RESCUE, SMALL1, SMALL3), left=LEFT_ALL),
    'v129': _case('four signal rows per lane; the rescue pass is on by default from here', volumes=129,
                  route=_rt('40', 1, 132, 4, rescue=True, s1='f32_8', s3='f32_8'), must=(GEMM_40, RESCUE, F32_8_1, F32_8_3), left=LEFT_ALL),
    'v150': _case('10 b0 + 40 + 60 + 40, three shells', protocol=P150, route=_rt('40', 1, 152, 4, rescue=True, s1='f32_8', s3='f32_8'),
                  must=(GEMM_40, RESCUE, F32_8_1, F32_8_3), errors=True, left=LEFT_ALL),
    'v160': _case('one window, for the last time', volumes=160, n_b0=10, route=_rt('40', 1, 160, 4, rescue=True, s1='f32_8', s3='f32_8'), must=(GEMM_40, RESCUE),
                  left=LEFT_ALL),
    'v161': _case('two windows of 84, the second holding 77 samples', volumes=161, n_b0=11, route=_rt('windows', 2, 84, 4, rescue=True, s1='f32_8', s3='f32_8'),
                  must=(GEMM_WIN, RESCUE), left=LEFT_ALL),
    'vLDS': _case('the last shape with its tile in LDS (218 volumes)', volumes='lds_edge', route=_rt('windows', 2, 112, 4, rescue=True, s1='f32_nw', s3='f32_8'),
                  must=(GEMM_WIN, RESCUE, PLAIN1, F32_8_3), must_not=(REPAIR, THIRD), left=LEFT_ALL),
    'vGT': _case('the first global-tile shape (219 volumes), still four rows per lane', volumes='lds_edge+1',
                 route=_rt('windows', 2, 112, 4, glob=True, rescue=True, third=True, s1='global', s2='global', s3='global'), must=(GEMM_WIN, REPAIR, RESCUE, THIRD),
                 left=LEFT_ALL),
    'v257': _case('eight rows per lane', volumes=257, route=_rt('windows', 2, 132, 8, glob=True, rescue=True, third=True, s1='global', s2='global', s3='global'),
                  must=(GEMM_WIN, REPAIR, RESCUE, THIRD), left=LEFT_ALL),
    'v288': _case('18 b0 + 90 + 180: the HCP-style shape', volumes=288, n_b0=18,
                  route=_rt('windows', 2, 144, 8, glob=True, rescue=True, third=True, s1='global', s2='global', s3='global'), must=(GEMM_WIN, REPAIR, RESCUE, THIRD),
                  errors=True, left=LEFT_ALL),
    'v512': _case('four windows of 128: the most the kernels take', volumes=512, n_b0=12,
                  route=_rt('windows', 4, 128, 8, glob=True, rescue=True, third=True, s1='global', s2='global', s3='global'), must=(GEMM_WIN, REPAIR, RESCUE, THIRD),
                  left=LEFT_ALL),
    # ---- passes forced, one switch per case
    'd145_rescue': _case('the rescue pass at 99 volumes', env={'AMX_RESCUE_FROM': '0'}, must=(RESCUE, 'k_nnls_gcert<3,rescue>'), left=('leftover_stage1', 'leftover_stage3')),
    'v150_rescue': _case('the rescue pass by the switch', protocol=P150, env={'AMX_RESCUE_FROM': '0'}, must=(RESCUE, 'k_nnls_gcert<3,rescue>'),
                         left=('leftover_stage1', 'leftover_stage3')),
    'd145_repair': _case('the second look of the NNLS certificates, tile in LDS', env={'AMX_GCERT_REPAIR': '1'}, must=(REPAIR, 'k_nnls_gcert<3,repair>'),
                         left=('leftover_stage1', 'leftover_stage3')),
    'v150_repair': _case('the second look at four rows per lane', protocol=P150, env={'AMX_GCERT_REPAIR': '1'}, must=(REPAIR, 'k_nnls_gcert<3,repair>'),
                         left=('leftover_stage1', 'leftover_stage3')),
    'd145_third': _case('the third LASSO certificate pass, every chunk; the seed solver goes to 26 atoms', env={'AMX_GCERT2_THIRD': '1'}, must=(THIRD,),
                        left=('leftover_lasso',)),
    'v150_third': _case('the third pass at four rows per lane', protocol=P150, env={'AMX_GCERT2_THIRD': '1'}, must=(THIRD,), left=('leftover_lasso',)),
    'd145_s2exact': _case('every stage-2 product by the exact pass', env={'AMX_S2_EXACT': '1'}, must=(GEMM_25_9, 'k_noddi_gemm<lasso>'), left=('leftover_lasso',)),
    'v150_s2exact': _case('the exact pass at four rows per lane', protocol=P150, env={'AMX_S2_EXACT': '1'}, must=(GEMM_40, 'k_noddi_gemm<lasso>'), left=('leftover_lasso',)),
    'v288_nothird': _case('the global-tile shape without the third pass', volumes=288, n_b0=18, env={'AMX_GCERT2_THIRD': '0'}, must=(WIDE, REPAIR), must_not=(THIRD,),
                          left=('leftover_lasso',)),
    'v288_norepair': _case('the global-tile shape without the second look', volumes=288, n_b0=18, env={'AMX_GCERT_REPAIR': '0'}, must=('k_nnls_gcert<1> ', THIRD),
                           must_not=(REPAIR,), left=('leftover_stage1', 'leftover_stage3')),
    # ---- lambdas
    # (at lambda2 = 1e-6, 19 .. 35 of 3 000 voxels are degenerate for the oracle, whatever the seed: the two seeds below leave 19 and 23, the
    #  names' own 26 and 29 of the 30 allowed)
    'd145_qr': _case('A-space QR solver, no LASSO seeds', lam=(0.5, 1e-6), route=_rt('25_9', 1, 100, 2, s2='qr'), must=('k_noddi<4|2> (all voxels)',),
                     must_not=(LSEED, 'k_lasso_gcert', 'k_noddi_lasso_big'), big_in_path=False, left=('leftover_stage1', 'leftover_stage3'), seed=2),
    'v150_qr': _case('QR at four rows per lane', protocol=P150, lam=(0.5, 1e-6), route=_rt('40', 1, 152, 4, rescue=True, s1='f32_8', s2='qr', s3='f32_8'),
                     must=('k_noddi<4|2> (all voxels)',), must_not=(LSEED, 'k_lasso_gcert', 'k_noddi_lasso_big'), big_in_path=False,
                     left=('leftover_stage1', 'leftover_stage3')),
    'v288_qr': _case('the global-tile QR build', volumes=288, n_b0=18, lam=(0.5, 1e-6),
                     route=_rt('windows', 2, 144, 8, glob=True, rescue=True, s1='global', s2='global', s3='global'), must=('k_noddi<4|2> (all voxels)',),
                     must_not=(LSEED, 'k_lasso_gcert', 'k_noddi_lasso_big'), big_in_path=False, left=('leftover_stage1', 'leftover_stage3'), seed=5),
    'd145_weak': _case('a weak lambda1: supports dense at every amplitude', lam=(0.05, 1e-3), route=_rt('25_9', 1, 100, 2), must=(BIG, LSEED), left=LEFT_ALL),
    'v150_weak': _case('dense supports at four rows per lane', protocol=P150, lam=(0.05, 1e-3), route=_rt('40', 1, 152, 4, rescue=True, s1='f32_8', s3='f32_8'),
                       must=(BIG, LSEED), left=LEFT_ALL),
    'v288_weak': _case('dense supports on the global tile', volumes=288, n_b0=18, lam=(0.05, 1e-3),
                       route=_rt('windows', 2, 144, 8, glob=True, rescue=True, third=True, s1='global', s2='global', s3='global'), must=(BIG, LSEED), left=LEFT_ALL),
    # ---- three large calls: what is keyed on voxel counts and has no switch (kLeftSmall1 / kLeftSmall3, kThirdFrom, the occ2 builds)
    'big99': _case('s1 the 12-wavefront fp64 build, s3 the fp64 build, both occ2 seed builds', n=BIG_N, signals='d145',
                   route=_rt('25_9', 1, 100, 2, s1='f64_12', s3='f64_nw'), must=('k_nnls_seed<1,8,occ2>', 'k_lasso_seed<occ2>', PLAIN1, PLAIN3),
                   must_not=(SMALL1, SMALL3, THIRD, RESCUE), left=LEFT_ALL),
    'big105': _case('9 b0 + 36 + 60: the third pass on by default', n=BIG_N, protocol=P105, signals='big105',
                    route=_rt('40', 1, 108, 2, third=True, s1='f64_12', s3='f64_nw'), must=(THIRD, 'k_lasso_seed<occ2>'), must_not=(SMALL1, SMALL3), left=LEFT_ALL),
    'big150': _case('the 8-wavefront float32 build in stages 1 and 3', n=BIG_N, protocol=P150, signals='v150',
                    route=_rt('40', 1, 152, 4, rescue=True, s1='f32_8', s3='f32_8'), must=(F32_8_1, F32_8_3, 'k_lasso_seed<occ2>'), must_not=(SMALL1, SMALL3),
                    left=LEFT_ALL),
}
SMALL_CASES = [k for k, c in CASES.items() if c['n'] == N_SMALL]
BIG_CASES = [k for k, c in CASES.items() if c['n'] != N_SMALL]
# cases that cannot have supports of more than 18 and of more than 64 atoms: 12 and 63 white-matter atoms; and lambda2 = 1e-6, where the
# LASSO's optimum is all but a vertex of the polytope (measured on these signals: at most 11 atoms at 99, 150 and 288 volumes)
NO_DENSE = ('d13', 'd64_l0', 'd145_qr', 'v150_qr', 'v288_qr')


def case_env(name):
    """the switches of a case: CHAIN + its own for the small ones, none for a large call (its size decides)"""
    c = CASES[name]
    return dict(c['env']) if c['n'] != N_SMALL else dict(CHAIN, **c['env'])


@functools.lru_cache(maxsize=None)
def lds_edge():
    """the largest volume count whose route on the default dictionary keeps the tile in LDS, from the route's own arithmetic"""
    from amico_amd import _capi
    for nS in range(256, 99, -1):
        if not _capi.noddi_route(nS, 144, nS - 9, 500, 0, 100_000)['global']:
            return nS
    raise AssertionError('no shape with its tile in LDS')


def case_protocol(name):
    c = CASES[name]
    if c['protocol'] is not None:
        return c['protocol']
    v = c['volumes']
    if v is None:
        return _protocol(99)
    if v == 'lds_edge':
        v = lds_edge()
    elif v == 'lds_edge+1':
        v = lds_edge() + 1
    return _protocol(v, c['n_b0'])


@functools.lru_cache(maxsize=4)
def _dictionary(protocol, grid):
    from amico_amd import synthetic as S
    sch = S.make_scheme(n_b0=protocol[0], shells=protocol[1], seed=0)
    ods = np.hstack((np.array([0.03, 0.06]), np.linspace(0.09, 0.99, grid[0] - 2)))
    K = S.noddi_kernels(sch, _htable()['dirs'], IC_VFs=np.linspace(0.1, 0.99, grid[1]), IC_ODs=ods)
    return sch, K


def dictionary(name):
    """(scheme, K) of a case, on the 500 LUT orientations"""
    return _dictionary(case_protocol(name), CASES[name]['grid'])


def case_seed(name):
    c = CASES[name]
    return c['seed'] if c['seed'] is not None else zlib.crc32((c['signals'] or name).encode()) % 10_000


@functools.lru_cache(maxsize=4)
def problem(name):
    """(sch, K, y, d, kind, amp) of a case's 3 000 voxels, read-only"""
    sch, K = dictionary(name)
    y, d, kind, amp = hard_signals(K, sch, case_seed(name))
    for a in (y, d, kind, amp):
        a.setflags(write=False)
    return sch, K, y, d, kind, amp


@functools.lru_cache(maxsize=4)
def reference(name):
    """the CPU oracle on a case's 3 000 voxels: {'x' [n, 3, n_atoms], 'estimates', 'rmse', 'nrmse'}, read-only"""
    from oracle import oracle
    c = CASES[name]
    sch, K, y, d, _, _ = problem(name)
    ref = oracle.noddi_fit(y, d, K, _htable()['htable'], sch.dwi_idx, c['lam'][0], c['lam'][1], is_exvivo=c['exvivo'], rmse=True, nrmse=True,
                           nthreads=NTHREADS, return_x=True)
    assert ref['err'] == 0, ref['err']
    for k in ('x', 'estimates', 'rmse', 'nrmse'):
        ref[k].setflags(write=False)
    return ref


def certificates(name, x):
    """kkt_certificates.noddi_certificates_per_voxel of the coefficients x [3000, 3, n_atoms] on a case's problem"""
    c = CASES[name]
    sch, K, y, d, _, _ = problem(name)
    return noddi_certificates_per_voxel(K, sch, _htable()['htable'], y, d, x, c['lam'][0], c['lam'][1], exvivo=c['exvivo'])


@functools.lru_cache(maxsize=4)
def reference_certificates(name):
    """certificates of the oracle's own coefficients (its stage-2 dual vector 'g2' decides which atoms are degenerate)"""
    return certificates(name, reference(name)['x'])


def kkt_failures(cert, bound=KKT):
    """voxels [bool n] that miss the certificate: min x >= 0 and |g_P| < bound s, g_Z < bound s in each stage, no stage-3 coefficient off
    the allowed set; an all-zero voxel passes only with every value exactly zero (its x is then exactly zero: checked by the caller)"""
    bad = cert['off3'] != 0.0
    for k in (1, 2, 3):
        bad |= (cert['min_x%d' % k] < 0) | ~(cert['gP%d' % k] < bound) | ~(cert['gZ%d' % k] < bound)
    return bad


def route_of(name):
    """_capi.noddi_route of a case's shape with the table's names: a call of 100 000 voxels (where the defaults run the chain; the small-call
    builds of the left-over kernels are those of 3 000 voxels too), a large call at its own size"""
    from amico_amd import _capi
    c = CASES[name]
    sch, K = dictionary(name)
    n = c['n'] if c['n'] != N_SMALL else 100_000
    rt = _capi.noddi_route(sch.nS, K['wm'].shape[0], len(sch.dwi_idx), 500, c['exvivo'], n, n, c['lam'][0], c['lam'][1])
    for mine, theirs in GEMM_KEYS.items():
        rt[mine] = rt[theirs]
    return rt
