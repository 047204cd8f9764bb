"""Every device route of CylinderZeppelinBall against the CPU oracle and the Kuhn-Tucker certificate of its own coefficients.

amx_czb_fit_device has two routes (amx_fit_dev.hip, czb_fit_dev).  The product path -- default ridge, no error maps, <= 32 atoms,
<= 160 volumes -- is k_czb_tables -> k_czb_project<25|40> -> k_czb_lane (+ the wavefront-per-voxel kernel over the overflow list);
everything else is k_czb, or k_czb_qr below lambda2 = 1e-6.  The tests of test_gpu_czb.py that have a reference ask for an error map
and therefore run k_czb.  Here every case first asserts its route from ctx.last_path(), then holds EVERY voxel to:

* the Kuhn-Tucker conditions of the device x (long-double residual): min x >= 0, max |g_P| < 1e-9, max g_Z < 1e-9;
* x against the oracle's x.  The objective is lambda2-strongly convex, so two feasible points with Kuhn-Tucker residuals <= 1e-9 are
  within 2 sqrt(n_atoms) 1e-9 / lambda2 of each other (czb_np.x_bound; 2.5e-9 at the defaults): that is the assertion.  Where the
  bound exceeds 1e-6 (weak ridges) x is not pinned to the digits the maps need, and A x is compared instead, with the thresholds of
  test_czb_without_a_ridge;
* supports equal to the oracle's, except atoms whose oracle coefficient / dual value is below that bound (a degenerate atom may sit on
  either side), on fewer than 1e-4 of the voxels (test_czb_np.py confirms the oracle's own supports against a long-double re-solve);
* maps: the device maps are czb_np.czb_maps of the DEVICE x to 1e-12 relative, and within |d| / (|ref| + 1e-3) < 1e-6 of the oracle's.

Non-finite signals must give NaN, directions outside the table zeros.
"""
import os

import numpy as np
import pytest

import czb_np as Z

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
IDS = np.array([5, 140, 260, 391, 470])
D_PAR = 0.6e-3
KKT = 1e-9            # the project's CylinderZeppelinBall threshold (test_gpu_czb.py, test_gpu_amplitude.py)
BATCH = 393_216       # voxels of one batch of the host-buffer route


def _dev():
    import torch
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------ dictionaries, once per module
_DICTS = {}


def _dictionary(htable500, nS=96, b0_at='start', n_atoms=26):
    """(K, Rs, n_perp) on the five orientations IDS: generated once per (scheme, atom set)"""
    key = (nS, b0_at, n_atoms)
    if key not in _DICTS:
        Rs, d_perps, d_isos = Z.atom_sets(n_atoms)
        K = Z.czb_kernels(Z.make_scheme(nS, b0_at, seed=nS), IDS, Rs, d_perps, d_isos, D_PAR, lut_dirs=htable500['dirs'])
        _DICTS[key] = (K, Rs, len(d_perps))
    return _DICTS[key]


@pytest.fixture(scope='module')
def full_dictionary(czb_fix, htable500):
    """all 500 orientations, the way bench.py --model czb builds them: Evaluation.generate_kernels + load_kernels on the fixture's
    96-volume scheme.  (K, Rs, n_perp, htable)"""
    import amico_amd
    from amico_amd import synthetic as S
    sch = S.SimpleScheme(czb_fix['scheme'])
    ae = amico_amd.Evaluation()
    ae.set_data(np.ones((2, 2, 2, sch.nS), dtype=np.float32), sch, np.ones((2, 2, 2), dtype=np.uint8))
    ae.set_model('CylinderZeppelinBall')
    ae.load_kernels(ae.generate_kernels(htable500['dirs']), htable500['dirs'])
    K = ae.KERNELS
    assert K['wmr'].shape == (21, 500, 96) and K['wmh'].shape == (4, 500, 96) and K['iso'].shape == (1, 96)
    return K, np.asarray(ae.model.Rs, dtype=np.float64), 4, np.ascontiguousarray(ae.htable).ravel()


def _problem(K, lut_dirs, ht, ori, rng, hard_share=1.0 / 3.0, snr=20.0):
    """directions inside the LUT cells ori, signals: the standard class, the last hard_share of the voxels the hard one"""
    ori = np.asarray(ori, dtype=np.int64)
    d = Z.dirs_in_cells(ori, lut_dirs, ht, rng)
    y = Z.czb_signals(K, ori, rng, snr=snr)
    h = int(round(len(ori) * (1.0 - hard_share)))
    if h < len(ori):
        y[h:] = Z.czb_signals(K, ori[h:], rng, hard=True)
    return y, d


# ------------------------------------------------------------------------------------------------ the fit and its checks
def _fit(ctx, L, y, d, lam1, lam2, f32=False, **kw):
    import torch
    from amico_amd import _capi
    yt = torch.from_numpy(y.astype(np.float32) if f32 else y).to(_dev())
    out = _capi.czb_fit_device(ctx, L, yt, torch.from_numpy(d).to(_dev()), lam1, lam2, return_x=True, **kw)
    return out


def _route(ctx, label, fast, nS=96, slow=None):
    """the route of the last call: fast -> k_czb_project<25|40> + k_czb_lane; otherwise the named wavefront-per-voxel kernel"""
    path = ctx.last_path()
    if fast:
        assert ('k_czb_project<25>' if nS <= 100 else 'k_czb_project<40>') in path and 'k_czb_lane' in path, (label, path)
        assert 'k_czb<' not in path and 'k_czb_qr<' not in path, (label, path)
    else:
        assert 'k_czb_lane' not in path and 'k_czb_project' not in path, (label, path)
        rows = 2 if nS <= 128 else (4 if nS <= 256 else 8)
        assert '%s<%d>' % (slow or 'k_czb', rows) in path, (label, path)
    return path


def _stats_clean(ctx, label, lane_holds_all=False):
    """no voxel at an iteration cap, none dropped.  lane_holds_all: a fast-path call on <= 26 atoms -- the smaller of the clamped and
    the passive set has at most 13 atoms, which a lane's factor holds, so no voxel may need the overflow-list kernel"""
    st = ctx.last_stats()
    assert st['itercap_voxels'] == 0 and st['guard_trips'] == 0 and st['overflow_voxels'] == 0, (label, st)
    if lane_holds_all:
        assert st['rerun_voxels'] == 0, (label, st)


def _check(label, K, Rs, n_perp, ht, y, d, est, x, lam1, lam2, nan_rows=(), bad_dir_rows=(), oracle_ref=None):
    """every voxel of one device result (est [n, 3], x [n, n_atoms], numpy) against the certificate and the oracle"""
    from amico_amd import synthetic as S
    from oracle import oracle
    n, n_atoms = x.shape
    ok = np.ones(n, bool)
    ok[list(nan_rows)] = False
    ok[list(bad_dir_rows)] = False
    for r in nan_rows:
        if r not in bad_dir_rows:
            assert np.isnan(est[r]).all() and np.isnan(x[r]).all(), (label, r, est[r])
    for r in bad_dir_rows:
        assert (est[r] == 0.0).all(), (label, r, est[r])
    rows = np.flatnonzero(ok)
    assert np.isfinite(est[rows]).all() and np.isfinite(x[rows]).all(), label
    lut = np.zeros(n, dtype=np.int64)
    lut[rows] = S.lut_indices(d[rows], ht)
    # Kuhn-Tucker conditions of the device coefficients
    g = Z.czb_gradient(K, lut, y, x, lam1, lam2, rows)
    P = x > 0
    gp = float(np.abs(g[rows][P[rows]]).max(initial=0.0))
    gz = float(g[rows][~P[rows]].max(initial=0.0))
    mn = float(x[rows].min())
    print('CZB %-46s n %6d  KKT |g_P| %.2e  g_Z %.2e  min x %.1e' % (label, len(rows), gp, gz, mn), end='')
    assert mn >= 0.0 and gp < KKT and gz < KKT, (label, gp, gz, mn)
    # maps (i): the map arithmetic alone, from the device x
    mine = Z.czb_maps(x[rows], Rs, n_perp)
    err = np.abs(est[rows] - mine) - (1e-12 * np.abs(mine) + 1e-300)
    assert (err <= 0.0).all(), (label, 'maps of the device x', int(rows[np.argmax(err.max(axis=1))]))
    # the oracle
    if oracle_ref is None:
        ref = oracle.czb_fit(y[rows], d[rows], K, Rs, ht, lam1, lam2, nthreads=NTHREADS, return_x=True)
        assert ref['err'] == 0, (label, ref['err'])
        xo, mo = ref['x'], ref['estimates']
    else:                                                  # (the caller's oracle fit of all voxels)
        xo, mo = oracle_ref['x'][rows], oracle_ref['estimates'][rows]
    bound = Z.x_bound(n_atoms, lam2)
    if bound <= 1e-6:
        dx = np.abs(x[rows] - xo).max(axis=1)
        print('  |x - oracle| %.2e (bound %.2e)' % (dx.max(), bound), end='')
        assert dx.max() <= bound, (label, float(dx.max()), bound, int(rows[dx.argmax()]))
        mism = (x[rows] > 0) != (xo > 0)
        need = np.flatnonzero(mism.any(axis=1))
        if len(need):
            go = Z.czb_gradient(K, lut[rows], y[rows], xo, lam1, lam2, need)
            degenerate = np.where(xo > 0, xo <= bound, np.abs(go) <= bound)
            assert degenerate[need][mism[need]].all(), (label, 'support differs on a non-degenerate atom', int(rows[need[0]]))
        print('  supports differ on %d' % len(need), end='')
        assert len(need) / len(rows) < 1e-4, (label, len(need), len(rows))
        rel = np.abs(est[rows] - mo) / (np.abs(mo) + 1e-3)
        print('  maps rel %.2e' % rel.max())
        assert rel.max() < 1e-6, (label, float(rel.max()), int(rows[rel.max(axis=1).argmax()]))
    else:
        ax = 0.0
        for grp in Z.by_direction(lut[rows]):
            A = Z.dictionary(K, lut[rows[grp[0]]])
            ax = max(ax, float(np.abs((x[rows[grp]] - xo[grp]) @ A.T).max()))
        print('  |A x - A x_oracle| %.2e (x bound %.1e: A x compared)' % (ax, bound))
        assert ax < (1e-8 if lam2 == 0.0 else 1e-4), (label, ax)
    return xo


def _run(label, ctx, L, K, Rs, n_perp, ht, y, d, lam1, lam2, fast, f32=False, slow=None, **kw):
    est, _, _, xd = _fit(ctx, L, y, d, lam1, lam2, f32=f32)
    ctx.sync()
    _route(ctx, label, fast, K['iso'].shape[1], slow)
    _stats_clean(ctx, label, fast and K['wmr'].shape[0] + K['wmh'].shape[0] + K['iso'].shape[0] <= 26)
    yw = y.astype(np.float32).astype(np.float64) if f32 else y
    est, x = est.cpu().numpy(), xd.cpu().numpy()
    _check(label, K, Rs, n_perp, ht, yw, d, est, x, lam1, lam2, **kw)
    return est, x


# ------------------------------------------------------------------------------------------------ 1. the default problem
@pytest.mark.parametrize('hard', [False, True], ids=['snr30', 'hard'])
def test_default_problem_100k_voxels_all_orientations(full_dictionary, htable500, hard):
    """the CylinderZeppelinBall leg of test_gpu_kkt.py: 100 000 voxels over all 500 orientations on the fast path, float64 and
    float32 signals in device memory (the float32 call against the oracle on the widened float32 values)"""
    from amico_amd import _capi, get_context
    K, Rs, n_perp, ht = full_dictionary
    rng = np.random.default_rng(101 + hard)
    n = 100_000
    ori = rng.integers(0, 500, n)
    y, d = _problem(K, htable500['dirs'], ht, ori, rng, hard_share=1.0 if hard else 0.0, snr=30.0)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    _run('default %s float64' % ('hard' if hard else 'SNR 30'), ctx, L, K, Rs, n_perp, ht, y, d, 0.0, 4.0, True)
    _run('default %s float32' % ('hard' if hard else 'SNR 30'), ctx, L, K, Rs, n_perp, ht, y, d, 0.0, 4.0, True, f32=True)
    L.close()


# ------------------------------------------------------------------------------------------------ 2. voxel counts, buckets
@pytest.mark.parametrize('n', [1, 63, 64, 65, 4097])
def test_fast_path_voxel_counts(full_dictionary, htable500, n):
    from amico_amd import _capi, get_context
    K, Rs, n_perp, ht = full_dictionary
    rng = np.random.default_rng(200 + n)
    y, d = _problem(K, htable500['dirs'], ht, rng.integers(0, 500, n), rng, hard_share=0.5 if n > 1 else 0.0)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    _run('n = %d' % n, ctx, L, K, Rs, n_perp, ht, y, d, 0.0, 4.0, True)
    L.close()


@pytest.mark.parametrize('layout', ['one_orientation_5000', '500_orientations_2_or_3_each'])
def test_fast_path_chunk_shapes(full_dictionary, htable500, layout):
    """one orientation with 5 000 voxels: several blocks of one chunk with a ragged tail; 500 orientations with 2 - 3 voxels each:
    every chunk shorter than a wavefront"""
    from amico_amd import _capi, get_context
    K, Rs, n_perp, ht = full_dictionary
    rng = np.random.default_rng(7)
    if layout == 'one_orientation_5000':
        ori = np.full(5000, 123)
    else:
        ori = rng.permutation(np.repeat(np.arange(500), 2 + (np.arange(500) % 2)))
    y, d = _problem(K, htable500['dirs'], ht, ori, rng)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    _run(layout, ctx, L, K, Rs, n_perp, ht, y, d, 0.0, 4.0, True)
    L.close()


def test_fast_path_writes_every_voxel(full_dictionary, htable500):
    """the fast-path twin of test_czb_fit_writes_every_voxel (whose AMX_F_RMSE keeps it on k_czb): outputs pre-filled with a
    sentinel, NaN / Inf signals and NaN directions mixed in; every voxel is written, and the finite ones are the oracle's"""
    import torch
    from amico_amd import _capi, get_context
    K, Rs, n_perp, ht = full_dictionary
    rng = np.random.default_rng(5)
    n = 30_011
    y, d = _problem(K, htable500['dirs'], ht, rng.integers(0, 500, n), rng)
    nan_rows = [11, 12, 4096, n - 1]
    y[11] = np.nan; y[12, 3] = np.inf; y[4096, 95] = -np.inf; y[n - 1] = np.nan
    bad = [17, n // 2, n - 2]
    d[bad] = np.nan
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    est, _, _, xd = _fit(ctx, L, y, d, 0.0, 4.0)
    with pytest.raises(RuntimeError, match=r'index out of bounds.*\[voxel 17\]'):
        ctx.sync()
    _route(ctx, 'sentinel', True)
    _stats_clean(ctx, 'sentinel', True)
    est, x = est.cpu().numpy(), xd.cpu().numpy()
    _check('NaN / Inf signals, NaN directions', K, Rs, n_perp, ht, y, d, est, x, 0.0, 4.0, nan_rows=nan_rows, bad_dir_rows=bad)
    yt, dt = torch.from_numpy(y).to(_dev()), torch.from_numpy(d).to(_dev())
    lib = _capi.lib()
    for fill in (-7.25, 0.0):
        e = torch.full((n, 3), fill, dtype=torch.float64, device=_dev())
        assert lib.amx_czb_fit_device(ctx._h, L._h, yt.data_ptr(), dt.data_ptr(), n, 0.0, 4.0, 0, e.data_ptr(), None, None, None) == 0
        with pytest.raises(RuntimeError, match=r'index out of bounds.*\[voxel 17\]'):
            ctx.sync()
        _route(ctx, 'sentinel %g' % fill, True)
        e = e.cpu().numpy()
        assert not (e == -7.25).any() and np.array_equal(e, est, equal_nan=True), fill
    L.close()


# ------------------------------------------------------------------------------------------------ 3. protocol lengths
PROTOCOLS = [(30, 'start'), (96, 'middle'), (100, 'single'), (101, 'start'), (128, 'middle'), (129, 'single'), (160, 'middle'),
             (161, 'start'), (256, 'single'), (257, 'middle'), (512, 'start')]


@pytest.mark.parametrize('nS,b0_at', PROTOCOLS)
def test_protocol_lengths(htable500, nS, b0_at):
    """k_czb_project<25> up to 100 volumes, <40> up to 160 (operand rows zero-padded to 100 / 160), k_czb with 4 / 8 rows per lane
    above; b0 volumes at the start, in the middle, a single one"""
    from amico_amd import _capi, get_context
    K, Rs, n_perp = _dictionary(htable500, nS, b0_at)
    ht = htable500['htable']
    rng = np.random.default_rng(300 + nS)
    n = 3000 if nS <= 160 else 1500
    y, d = _problem(K, htable500['dirs'], ht, IDS[rng.integers(len(IDS), size=n)], rng)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    _run('nS = %d, b0 %s' % (nS, b0_at), ctx, L, K, Rs, n_perp, ht, y, d, 0.0, 4.0, nS <= 160)
    L.close()


# ------------------------------------------------------------------------------------------------ 4. dictionary sizes
@pytest.mark.parametrize('n_atoms', [11, 26, 31, 32, 33, 48, 64])
def test_dictionary_sizes(htable500, n_atoms):
    """<= 32 atoms: the fast path; a lane's factor holds 13 atoms, so with 31 / 32 atoms a voxel whose clamped AND passive sets both
    exceed 13 must go through the overflow list to the wavefront-per-voxel kernel -- asserted on the inputs, by the oracle's x, to be
    at least 1 % of the voxels.  33 - 64 atoms: k_czb, main pass with 32 passive atoms, re-run pass with 64."""
    from amico_amd import _capi, get_context
    from oracle import oracle
    K, Rs, n_perp = _dictionary(htable500, 96, 'start', n_atoms)
    ht = htable500['htable']
    rng = np.random.default_rng(400 + n_atoms)
    n = 3000
    y, d = _problem(K, htable500['dirs'], ht, IDS[rng.integers(len(IDS), size=n)], rng, hard_share=0.5)
    ref = oracle.czb_fit(y, d, K, Rs, ht, 0.0, 4.0, nthreads=NTHREADS, return_x=True)
    xo = ref['x']
    if n_atoms in (31, 32):
        npos = (xo > 0).sum(axis=1)
        beyond = int(((npos > 13) & (n_atoms - npos > 13)).sum())
        print('CZB %d atoms: %d of %d voxels beyond a lane (both sets > 13 atoms)' % (n_atoms, beyond, n))
        assert beyond >= 0.01 * n, (n_atoms, beyond)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    _run('%d atoms' % n_atoms, ctx, L, K, Rs, n_perp, ht, y, d, 0.0, 4.0, n_atoms <= 32, oracle_ref=ref)
    st = ctx.last_stats()
    assert st['overflow_voxels'] == 0, st                                         # nothing dropped
    if n_atoms in (31, 32):
        assert st['rerun_voxels'] >= beyond, (st, beyond)                         # ... and the overflow-list kernel did serve them
    L.close()


# ------------------------------------------------------------------------------------------------ 5. lambda1 > 0
@pytest.mark.parametrize('lam1', [0.05, 0.5, 5.0])
@pytest.mark.parametrize('route', ['fast', 'k_czb'])
def test_lambda1(htable500, lam1, route):
    """c = A'y - lambda1, z0 = B y - lambda1 M 1 on the fast path; lambda1 = 5 clamps most atoms (the passive-form branch of
    k_czb_lane, all-zero solutions).  k_czb: the same problems on a 33-atom dictionary."""
    from amico_amd import _capi, get_context
    n_atoms = 26 if route == 'fast' else 33
    K, Rs, n_perp = _dictionary(htable500, 96, 'start', n_atoms)
    ht = htable500['htable']
    rng = np.random.default_rng(500)
    n = 4000
    y, d = _problem(K, htable500['dirs'], ht, IDS[rng.integers(len(IDS), size=n)], rng)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    est, x = _run('lambda1 = %g, %s' % (lam1, route), ctx, L, K, Rs, n_perp, ht, y, d, lam1, 4.0, route == 'fast')
    npos = (x > 0).sum(axis=1)
    print('CZB lambda1 = %g: passive atoms per voxel mean %.1f, all-zero voxels %d' % (lam1, npos.mean(), int((npos == 0).sum())))
    if lam1 == 5.0 and route == 'fast':
        # more than 13 clamped atoms: the lane factors the passive set instead (the `!zform` branch); all-zero optima
        assert (npos < n_atoms - 13).sum() >= 0.05 * n and (npos == 0).any(), (int((npos < n_atoms - 13).sum()), int((npos == 0).sum()))
    L.close()


# ------------------------------------------------------------------------------------------------ 6. lambda2 routes, table cache
def test_lambda2_routes_and_table_cache(htable500):
    """one uploaded dictionary, lambda2 = 4, 1e-2, 4, 9.9e-3, 1e-4, 1e-6, 9e-7, 4: the tables of the fast path are cached per lambda2
    and rebuilt on change -- the three lambda2 = 4 results are bit-identical; the route of every call"""
    from amico_amd import _capi, get_context
    K, Rs, n_perp = _dictionary(htable500)
    ht = htable500['htable']
    rng = np.random.default_rng(600)
    n = 4000
    y, d = _problem(K, htable500['dirs'], ht, IDS[rng.integers(len(IDS), size=n)], rng)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    at4 = []
    for lam2, route in ((4.0, 'fast'), (1e-2, 'fast'), (4.0, 'fast'), (9.9e-3, 'k_czb'), (1e-4, 'k_czb'), (1e-6, 'k_czb'),
                        (9e-7, 'k_czb_qr'), (4.0, 'fast')):
        est, x = _run('lambda2 = %g' % lam2, ctx, L, K, Rs, n_perp, ht, y, d, 0.0, lam2, route == 'fast', slow=route)
        if lam2 == 4.0:
            at4.append((est, x))
    for est, x in at4[1:]:
        assert np.array_equal(est, at4[0][0]) and np.array_equal(x, at4[0][1])
    L.close()


# ------------------------------------------------------------------------------------------------ 7. amplitudes
def test_fast_path_is_scale_equivariant(htable500):
    """test_czb_is_scale_equivariant without error maps, i.e. on the fast path: maps invariant (the rules of
    test_gpu_amplitude._compare_maps), Kuhn-Tucker residuals below 1e-9 c, the same kernels at every scale"""
    from amico_amd import _capi, get_context
    from test_gpu_amplitude import SCALES, _compare_maps
    K, Rs, n_perp = _dictionary(htable500)
    ht = htable500['htable']
    rng = np.random.default_rng(13)
    n = 20_000
    ori = IDS[rng.integers(len(IDS), size=n)]
    y, d = _problem(K, htable500['dirs'], ht, ori, rng, hard_share=0.0)
    y = y.astype(np.float32).astype(np.float64)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    ref = None
    for c in (1.0,) + SCALES:
        est, _, _, xd = _fit(ctx, L, c * y, d, 0.0, 4.0)
        ctx.sync()
        path = _route(ctx, ('amplitude', c), True)
        _stats_clean(ctx, ('amplitude', c), True)
        est, x = est.cpu().numpy(), xd.cpu().numpy()
        gp, gz, mn = Z.czb_certificate(K, ori, c * y, x, 0.0, 4.0)
        print('CZB fast path c = 2^%-3d KKT |g_P| / c %.2e  g_Z / c %.2e' % (int(np.log2(c)), gp / c, gz / c))
        assert mn >= 0.0 and gp < KKT * c and gz < KKT * c, (c, gp, gz)
        if ref is None:
            ref = (est, x, path)
            _check('amplitude 1', K, Rs, n_perp, ht, y, d, est, x, 0.0, 4.0)
            continue
        assert path == ref[2], (c, path, ref[2])
        den = np.abs(ref[0]) + 1e-3
        _compare_maps('CylinderZeppelinBall fast path v/a/d (rel)', c, est / den, ref[0] / den)
        assert ((x > 0) == (ref[1] > 0)).all(axis=1).mean() >= 0.9999, c
    L.close()


# ------------------------------------------------------------------------------------------------ 8. host buffers, several batches
def test_host_buffers_above_one_batch(full_dictionary, htable500):
    """450 000 voxels from host arrays (float64 and float32) travel in more than one batch: bit-identical to the one-launch call on
    device-resident signals, as test_small_models_pipelined_host_path asserts for FreeWater and SANDI"""
    import torch
    from amico_amd import _capi, get_context
    K, Rs, n_perp, ht = full_dictionary
    rng = np.random.default_rng(800)
    n = 450_000
    assert n > BATCH
    ori = rng.integers(0, 500, n)
    d = Z.dirs_in_cells(ori, htable500['dirs'], ht, rng)
    y = Z.czb_signals(K, ori, rng, snr=30.0)
    y32 = y.astype(np.float32)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    dt = torch.from_numpy(d).to(_dev())
    sel = np.arange(0, n, 50)
    for name, yh in (('float64', y), ('float32', y32)):
        devr, _, _, xd = _capi.czb_fit_device(ctx, L, torch.from_numpy(yh).to(_dev()), dt, 0.0, 4.0, return_x=True)
        ctx.sync()
        _route(ctx, ('device', name), True)
        _stats_clean(ctx, ('device', name), True)
        devr = devr.cpu().numpy()
        host = _capi.czb_fit(ctx, L, yh, d, 0.0, 4.0)[0]
        _route(ctx, ('host', name), True)
        assert np.isfinite(host).all() and np.array_equal(host, devr), name
        # ... and that result is the oracle's, on every 50th voxel
        _check('450 000 voxels, %s, sample' % name, K, Rs, n_perp, ht, yh[sel].astype(np.float64), d[sel], devr[sel], xd.cpu().numpy()[sel], 0.0, 4.0)
    L.close()


# ------------------------------------------------------------------------------------------------ 9. fast against slow
def test_fast_and_slow_routes_agree(htable500):
    """the same 20 000 voxels without flags (fast) and with rmse=True (k_czb): x within the derived bound of each other, and the RMSE
    map of the second call is that of the coefficients of the first -- the error map a user gets belongs to the maps they get"""
    from amico_amd import _capi, get_context
    K, Rs, n_perp = _dictionary(htable500)
    ht = htable500['htable']
    rng = np.random.default_rng(900)
    n = 20_000
    ori = IDS[rng.integers(len(IDS), size=n)]
    y, d = _problem(K, htable500['dirs'], ht, ori, rng)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, Rs, ht)
    est_f, x_f = _run('fast', ctx, L, K, Rs, n_perp, ht, y, d, 0.0, 4.0, True)
    est, r, _, xd = _fit(ctx, L, y, d, 0.0, 4.0, rmse=True)
    ctx.sync()
    _route(ctx, 'slow', False)
    _stats_clean(ctx, 'slow')
    x_s, r = xd.cpu().numpy(), r.cpu().numpy()
    bound = Z.x_bound(x_f.shape[1], 4.0)
    assert np.abs(x_f - x_s).max() <= bound, (float(np.abs(x_f - x_s).max()), bound)
    rel = np.abs(est.cpu().numpy() - est_f) / (np.abs(est_f) + 1e-3)
    assert rel.max() < 1e-6, rel.max()
    rm = np.zeros(n)
    for grp in Z.by_direction(ori):
        A = Z.dictionary(K, ori[grp[0]])
        rm[grp] = np.sqrt(((y[grp] - x_f[grp] @ A.T) ** 2).mean(axis=1))
    assert np.abs(r - rm).max() < 1e-9, float(np.abs(r - rm).max())
    L.close()
