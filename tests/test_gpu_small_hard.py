"""Every device route of FreeWater and SANDI on hard voxels, each voxel held to its own Kuhn-Tucker certificate and to the CPU oracle.

The routes and the shape that selects each are the tables small_np.FW_CASES / SANDI_CASES; every case first asserts its kernel from
ctx.last_path().  The signals are small_np.hard_mix: every third voxel is all-zero, exactly one atom, pure noise, negated, signed,
constant, the uniform mixture ..., and amplitudes 2^-20, 1 and 2^20 sit side by side in every wavefront.  FreeWater runs three
orientations of 2 100, 835 and 65 voxels (three 1 024-voxel units of the fused kernel with a wrapped 5-slot ring and a ragged tile;
one unit; one tile + 1 voxel), SANDI 3 000 voxels.  With s = max|y| of the voxel, EVERY voxel is held to:

* the certificate of the device x (long-double residual): min x >= 0, max |g_P| < 1e-9 s, max g_Z < 1e-9 s -- the project's W_P_TOL /
  W_Z_TOL per voxel and relative; an all-zero voxel has x exactly 0 (small_np.kkt_ok);
* x against the oracle: |x - x_oracle| <= czb_np.x_bound(n_atoms, lambda2, s).  Where that bound exceeds 1e-6 s, or lambda2 = 0, A x is
  compared instead: within 1e-4 s, 1e-8 s at lambda2 = 0 (the thresholds of test_czb_without_a_ridge, relative);
* supports equal to the oracle's except on degenerate atoms (small_np.degenerate with that bound);
* maps: the device maps are small_np.fw_maps / sandi_maps of the DEVICE x to 1e-12 relative (FreeWater's second map is 1 - v: it
  inherits the rounding of v, 2 eps absolute, which no relative bound covers when v is near 1 -- it gets 4 eps on top), and within
  1e-6 of the oracle's (small_np.map_distance), nothing left out -- a voxel that misses is taken to the long-double re-solve, and
  where the oracle itself is off that by more than 1e-8 the device is held to the re-solve instead, to the same 1e-6 (_adjudicate);
  SANDI at ridges <= 1e-9: 1e-4 (WEAK_RIDGE_MAP_TOL, with its reason);
* itercap_voxels == 0 and overflow_voxels == 0;
* two more voxels, one with a NaN sample and one with +Inf in the last sample, give NaN maps and change no other voxel's bits;
* error maps where the case asks: |rmse - rmse_ld(device x)| <= 1e-9 rmse + 3e-8 rms(y), the floor test_gpu_amplitude._compare_scaled
  documents for Gram-form residuals; NRMSE likewise (floor 3e-8); FreeWater's corrected rows are numpy's from the device x_iso to
  8 eps s (one rounding per operation).

test_small_hard.py shows on the CPU that the oracle meets this standard with three digits to spare on the same signals.

MEASURED on an MI355X (profiles/small_hard_kkt.txt): all 35 cases pass; worst gP / s 1.4e-12 (k_sandi_rows), gZ / s 1.4e-14, x or A x at
most 5e-6 of its bound.  Two kernel changes came out of it: the zero-residual exit of the wavefront solvers at
lambda1 = lambda2 = 0, and the dual tolerance of the lane solvers, which was an absolute 1e-12 and left clamped atoms with g_Z up to
5.7e-6 s on voxels of amplitude 2^-20."""
import functools
import os
import zlib

import numpy as np
import pytest

import czb_np as Z
import small_np as N

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
EPS = np.finfo(np.float64).eps
# SANDI with a ridge of 1e-9 or less: the maps against a reference are held to 1e-4, not 1e-6.  The dictionaries have rank <= shells + 1
# < n_atoms, so along the directions A does not see x is held by the ridge alone: two points whose Kuhn-Tucker residuals are r lie
# within 2 sqrt(n) r / lambda2 of each other.  The oracle's residual (<= 4e-13 s, test_small_hard.py) gives 3e-3 s at 1e-9; measured on
# the 3 000 voxels of these cases, the oracle ALONE is off the long-double re-solve by 1.9e-5 (wave2), 2.5e-6 (long_edge) and 3.7e-7
# (lane15_edge) in a map, and a device x with residuals of 2e-14 s is off the re-solve by 1.9e-6 (long_edge).  1e-4 is the figure the
# A x comparison uses at such ridges; the certificate, A x and the maps of the device's own x keep their bounds.
WEAK_RIDGE_MAP_TOL = 1e-4
FW_RUNS = [(name, lam) for name, c in N.FW_CASES.items() for lam in c['lams']]
SANDI_RUNS = [(name, lam) for name, c in N.SANDI_CASES.items() for lam in c['lams']]


def _ids(runs):
    return ['%s-%g-%g' % (n, l[0], l[1]) for n, l in runs]


def _seed(name):
    return zlib.crc32(name.encode()) % 10_000


# ------------------------------------------------------------------------------------------------ problems and references, once
@functools.lru_cache(maxsize=None)
def _fw_problem(name):
    c = N.FW_CASES[name]
    _, K = N.fw_case_dictionary(c)
    y, d, lut, kind = N.fw_problem(K, seed=_seed(name), f32=c['f32'])
    for a in (y, d, lut, kind):
        a.setflags(write=False)
    return K, y, d, lut, kind


@functools.lru_cache(maxsize=None)
def _fw_reference(name, lam):
    K, y, d, lut, _ = _fw_problem(name)
    xo, mo = N.fw_reference(K, N.FW_CASES[name], lam, y, d, lut, nthreads=NTHREADS)
    xo.setflags(write=False); mo.setflags(write=False)
    return xo, mo


@functools.lru_cache(maxsize=None)
def _sandi_problem(name):
    c = N.SANDI_CASES[name]
    _, K, Rs, d_in, d_isos = N.sandi_case_dictionary(c)
    y, kind = N.sandi_problem(K, 3000, seed=_seed(name), f32=c['f32'], exact=c['exact'])
    y.setflags(write=False); kind.setflags(write=False)
    return K, Rs, d_in, d_isos, y, kind


@functools.lru_cache(maxsize=None)
def _sandi_reference(name, lam):
    K, Rs, d_in, d_isos, y, _ = _sandi_problem(name)
    xo, mo = N.sandi_reference(K, Rs, d_in, d_isos, lam, y, nthreads=NTHREADS)
    xo.setflags(write=False); mo.setflags(write=False)
    return xo, mo


def _with_bad_voxels(y):
    """two more voxels behind the others: copies of voxels 1 and 2 with a NaN sample / +Inf in the last sample"""
    bad = np.array(y[[1, 2]])
    bad[0, 3] = np.nan
    bad[1, -1] = np.inf
    return np.ascontiguousarray(np.vstack([y, bad]))


def _route(path, c, label):
    want = c['route']
    assert want in path, (label, path)
    if want == N.FW_LANE:
        assert 'refill' not in path and 'fused' not in path and 'wavefront per voxel' not in path, (label, path)
    if want == N.S_LANE:
        assert 'k_sandi_rows' not in path and 'wavefront per voxel' not in path and 'k_sandi_gram' not in path, (label, path)
    if want in (N.FW_WAVE, N.S_WAVE):
        assert 'lane' not in path and 'refill' not in path and 'fused' not in path and 'rows' not in path, (label, path)


# ------------------------------------------------------------------------------------------------ the checks every case shares
def _check(label, route, groups, y, kind, x, maps, maps_of_x, xo, mo, lam, n_atoms, maps_of_solver_x=None, map_tol=1e-6):
    """x: the solver's coefficients of the device (SANDI: before the rescaling); maps_of_x(x) restates the maps from them.
    Returns what it found wrong, one entry per property (the caller asserts that nothing was): a failing case reports all of them"""
    found = []
    lam1, lam2 = lam
    n = len(y)
    s = N.scale_of(y)
    if not (np.isfinite(x).all() and np.isfinite(maps).all()):
        return ['non-finite results on %d finite voxels' % int((~np.isfinite(x).all(axis=1) | ~np.isfinite(maps).all(axis=1)).sum())]
    # Kuhn-Tucker conditions of the device coefficients, per voxel
    ok, gps, gzs = np.zeros(n, bool), np.zeros(n), np.zeros(n)
    for rows, A in groups:
        ok[rows], gps[rows], gzs[rows] = N.kkt_ok(A, y[rows], x[rows], lam1, lam2)
    # x (or A x) against the oracle
    unit = Z.x_bound(n_atoms, lam2)
    by_x = unit <= 1e-6
    if by_x:
        ratio = np.abs(x - xo).max(axis=1) / np.where(s > 0, unit * s, 1.0)
    else:
        thr = 1e-8 if lam2 == 0.0 else 1e-4
        ratio = np.zeros(n)
        for rows, A in groups:
            ratio[rows] = np.abs((x[rows] - xo[rows]) @ A.T).max(axis=1) / np.where(s[rows] > 0, thr * s[rows], 1.0)
    live = s > 0
    w = int(np.argmax(np.where(live, np.maximum(np.maximum(gps, gzs) / N.KKT, ratio), 0.0)))
    print('SMALLHARD %-24s %-40s gP/s %.2e  gZ/s %.2e  %s %.2e  worst: %s x %g' %
          (label, route, gps[live].max(), gzs[live].max(), '|dx|/bound' if by_x else '|A dx|/bound', ratio.max(), N.KINDS[kind[w]], s[w]))
    if x[~live].any():
        found.append('an all-zero voxel with a non-zero x')
    if not ok.all():
        found.append(('certificate', 'voxels', int((~ok).sum()), 'first', int(np.flatnonzero(~ok)[0]), 'gP/s', float(gps.max()), 'gZ/s', float(gzs.max()),
                      'min x', float(x.min()), sorted(set(N.KINDS[k] for k in kind[~ok])), 'scales', sorted(set(np.round(np.log2(s[~ok & live])).astype(int)))[:6]))
    if not (ratio <= 1.0).all():
        bad = ratio > 1.0
        found.append(('x against the oracle', 'voxels', int(bad.sum()), 'worst', float(ratio.max()), int(ratio.argmax()), sorted(set(N.KINDS[k] for k in kind[bad]))))
    # supports
    if np.isfinite(unit):
        mism = (x > 0) != (xo > 0)
        for rows, A in groups:
            need = rows[mism[rows].any(axis=1)]
            if len(need):
                go = N.gradient(A, y[need], xo[need], lam1, lam2)
                deg = N.degenerate(xo[need], go, unit * s[need])
                if not deg[mism[need]].all():
                    w = need[(mism[need] & ~deg).any(axis=1)]
                    found.append(('support differs on a non-degenerate atom', 'voxels', len(w), int(w[0]), sorted(set(N.KINDS[k] for k in kind[w]))))
    # maps: the arithmetic alone, then against the oracle
    mine = maps_of_x(x)
    tol = 1e-12 * np.abs(mine) + 1e-300
    if maps.shape[1] in (2, 4):
        tol[:, 1] += 4 * EPS
    err = np.abs(maps - mine) - tol
    if not (err <= 0.0).all():
        w = int(err.max(axis=1).argmax())
        found.append(('maps of the device x', 'voxels', int((err > 0).any(axis=1).sum()), w, maps[w].tolist(), mine[w].tolist()))
    dm = N.map_distance(maps, mo)
    if not dm.max() < map_tol and lam2 > 0.0:
        dm = _adjudicate(groups, y, maps, mo, dm, xo, lam, maps_of_solver_x or maps_of_x, map_tol)
    if not dm.max() < map_tol:
        bad = ~(dm < map_tol)
        found.append(('maps against the oracle', 'voxels', int(bad.sum()), 'worst', float(dm.max()), int(dm.argmax()), sorted(set(N.KINDS[k] for k in kind[bad])),
                      'scales', sorted(set(np.round(np.log2(s[bad & live])).astype(int)))[:6]))
    return found


def _adjudicate(groups, y, maps, mo, dm, xo, lam, maps_of_solver_x, map_tol):
    """A voxel whose maps miss the oracle's by 1e-6 is taken to the long-double re-solve (czb_np.czb_resolve), which is the more exact
    of the two references: where the ORACLE's maps are off the re-solve's by more than the 1e-8 that test_small_hard.py holds them to,
    the voxel's distance becomes that of the device maps from the re-solve's -- the bound stays what it was.  Reason: the oracle's own
    Kuhn-Tucker residual, <= 4e-13 s, leaves its x uncertain by residual / lambda2 along directions the dictionary does not pin; for
    SANDI (rank <= shells + 1 < n_atoms) at lambda2 <= 1e-9 that is 4e-4 s, and on 3 000 voxels the oracle alone is off the re-solve
    by 1.9e-5 (100 x 15, 5e-10), 3.7e-7 (6 x 15, 1e-9) and 2.5e-6 (129 x 15, 1e-9) on a handful of ordinary voxels."""
    dm = dm.copy()
    for rows, A in groups:
        for v in rows[~(dm[rows] < map_tol)]:
            try:
                xr, _ = Z.czb_resolve(A, y[v], lam[0], lam[1])
            except RuntimeError:
                try:
                    xr, _ = Z.czb_resolve(A, y[v], lam[0], lam[1], start=xo[v] > 0)
                except RuntimeError:
                    continue
            mr = maps_of_solver_x(xr[None])
            if N.map_distance(mr, mo[v:v + 1])[0] > 1e-8:
                dm[v] = N.map_distance(maps[v:v + 1], mr)[0]
    return dm


def _check_errors(label, groups, y, x_err, rmse, nrmse):
    """x_err: the coefficients the error maps are made of (SANDI: the rescaled ones, against the normalised dictionary)"""
    rms = np.sqrt((y * y).mean(axis=1))
    found = []
    for rows, A in groups:
        if rmse is not None:
            ref = N.rmse_ld(A, y[rows], x_err[rows])
            bad = ~(np.abs(rmse[rows] - ref) <= 1e-9 * ref + 3e-8 * rms[rows])
            if bad.any():
                found.append(('rmse', 'voxels', int(bad.sum()), int(rows[bad][0]), float(rmse[rows][bad][0]), float(ref[bad][0]), float(rms[rows][bad][0])))
        if nrmse is not None:
            ref = N.nrmse_ld(A, y[rows], x_err[rows])
            bad = ~(np.abs(nrmse[rows] - ref) <= 1e-9 * ref + 3e-8)
            if bad.any():
                found.append(('nrmse', 'voxels', int(bad.sum()), int(rows[bad][0]), float(nrmse[rows][bad][0]), float(ref[bad][0])))
    return found


def _stats_clean(ctx, found):
    st = ctx.last_stats()
    if not (st['itercap_voxels'] == 0 and st['overflow_voxels'] == 0):
        found.append(('solver statistics', st))


def _same_bits(label, clean, dirty, n):
    """the run with the two bad voxels behind: NaN maps for them, every other voxel's results (maps, error maps, corrected rows,
    coefficients) to the last bit what they were without them"""
    found = []
    for k, (a, b) in enumerate(zip(clean, dirty)):
        if a is None:
            continue
        a, b = a.cpu().numpy(), b.cpu().numpy()
        if k == 0 and not np.isnan(b[n:]).all():
            found.append(('maps of the bad voxels', b[n:].tolist()))
        if not np.array_equal(a, b[:n]):
            w = np.flatnonzero((a != b[:n]).reshape(n, -1).any(axis=1))
            found.append(('a bad voxel changed others', 'output', k, 'voxels', len(w), int(w[0]), float(np.abs(a - b[:n]).max())))
    return found


# ------------------------------------------------------------------------------------------------ FreeWater
@pytest.mark.parametrize('name,lam', FW_RUNS, ids=_ids(FW_RUNS))
def test_freewater_route_on_hard_voxels(name, lam, amx_env):
    import torch
    from amico_amd import _capi, get_context
    c = N.FW_CASES[name]
    if c['env']:
        amx_env(**c['env'])
    K, y, d, lut, kind = _fw_problem(name)
    xo, mo = _fw_reference(name, lam)
    n, n_perp = len(y), c['n_perp']
    label = '%s (%g, %g)' % (name, lam[0], lam[1])
    dev = torch.device('cuda', 0)
    dt = np.float32 if c['f32'] else np.float64
    ctx = get_context()
    L = _capi.upload_freewater(ctx, K, N._htable()['htable'])
    want = dict(rmse=c['rmse'], nrmse=c['nrmse'], corrected=c['corrected'])

    def fit(yy, dd):
        out = _capi.freewater_fit_device(ctx, L, torch.from_numpy(np.array(yy, dtype=dt)).to(dev), torch.from_numpy(np.array(dd)).to(dev),
                                         lam[0], lam[1], c['mouse'], return_x=True, **want)
        ctx.sync()
        _route(ctx.last_path(), c, label)
        _stats_clean(ctx, found)
        return out
    found = []
    clean = fit(y, d)
    dirty = fit(_with_bad_voxels(y), np.vstack([d, d[[1, 2]]]))
    L.close()
    found += _same_bits(label, clean, dirty, n)
    est, rmse, nrmse, yc, xd = [None if t is None else t.cpu().numpy() for t in clean]
    groups = N.fw_groups(K, lut)
    found += _check(label, c['route'], groups, y, kind, xd, est, lambda x: N.fw_maps(x, n_perp, c['mouse']), xo, mo, lam, xd.shape[1])
    found += _check_errors(label, groups, y, xd, rmse, nrmse)
    if yc is not None:
        ref = N.fw_corrected(y, xd[:, n_perp:], K['CSF'].astype(np.float64))
        bad = ~(np.abs(yc - ref) <= 8 * EPS * N.scale_of(y)[:, None]).all(axis=1)
        if bad.any():
            found.append(('corrected rows', 'voxels', int(bad.sum()), int(np.flatnonzero(bad)[0]), float(np.abs(yc - ref).max())))
        assert (yc == 0).any()
    assert not found, (label, found)


# ------------------------------------------------------------------------------------------------ SANDI
@pytest.mark.parametrize('name,lam', SANDI_RUNS, ids=_ids(SANDI_RUNS))
def test_sandi_route_on_hard_voxels(name, lam, amx_env):
    import torch
    from amico_amd import _capi, get_context
    c = N.SANDI_CASES[name]
    if c['env']:
        amx_env(**c['env'])
    K, Rs, d_in, d_isos, y, kind = _sandi_problem(name)
    xo, mo = _sandi_reference(name, lam)
    n = len(y)
    label = '%s (%g, %g)' % (name, lam[0], lam[1])
    dev = torch.device('cuda', 0)
    dt = np.float32 if c['f32'] else np.float64
    ctx = get_context()
    L = _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)

    def fit(yy):
        out = _capi.sandi_fit_device(ctx, L, torch.from_numpy(np.array(yy, dtype=dt)).to(dev), lam[0], lam[1], rmse=c['rmse'], nrmse=c['nrmse'], return_x=True)
        ctx.sync()
        _route(ctx.last_path(), c, label)
        _stats_clean(ctx, found)
        return out
    found = []
    clean = fit(y)
    dirty = fit(_with_bad_voxels(y))
    L.close()
    found += _same_bits(label, clean, dirty, n)
    est, rmse, nrmse, xd = [None if t is None else t.cpu().numpy() for t in clean]
    norms = K['norms'][None, :]
    groups = [(np.arange(n), N.sandi_matrix(K))]
    # (the device returns the rescaled coefficients, models.pyx:1570-1571: the maps restate from them, the certificate undoes it)
    found += _check(label, c['route'], groups, y, kind, xd / norms, est, lambda x: N.sandi_maps(xd, len(Rs), len(d_in), Rs, d_in, d_isos), xo, mo, lam,
                    xd.shape[1], maps_of_solver_x=lambda x: N.sandi_maps(x * norms, len(Rs), len(d_in), Rs, d_in, d_isos),
                    map_tol=WEAK_RIDGE_MAP_TOL if 0.0 < lam[1] <= 1e-9 else 1e-6)
    found += _check_errors(label, groups, y, xd, rmse, nrmse)
    assert not found, (label, found)
