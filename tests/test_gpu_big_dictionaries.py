"""FreeWater, SANDI and CylinderZeppelinBall on dictionaries of 65 .. 256 atoms (k_enet_big, amx_enet_big.hip) on hard voxels, each voxel
held to its own Kuhn-Tucker certificate and to the CPU oracle.  Without that route every case here fails at the dictionary upload.

The shapes, signals and references are big_np's (test_big_dictionaries.py shows on the CPU that the oracle alone meets the certificate on
them).  The standard is the one test_gpu_small_hard.py states, restated here.  With s = max|y| of the voxel, EVERY voxel is held to:

* the certificate of the device x (long-double residual): min x >= 0, max |g_P| < 1e-9 s, max g_Z < 1e-9 s; an all-zero voxel has x exactly
  0 (small_np.kkt_ok);
* x against the oracle: |x - x_oracle| <= czb_np.x_bound(n_atoms, lambda2, s).  Where that bound exceeds 1e-6 s, A x is compared instead,
  within 1e-4 s (1e-8 s at lambda2 = 0);
* supports equal to the oracle's except on degenerate atoms (small_np.degenerate with that bound);
* maps: the device maps are the model's arithmetic on the DEVICE x to 1e-12 relative (+ 4 eps on FreeWater's 1 - v), and within 1e-6 of
  the oracle's (small_np.map_distance), nothing left out; a voxel that misses is taken to the long-double re-solve, and where the oracle
  itself is off that by more than 1e-8 the device is held to the re-solve instead, to the same 1e-6 (_adjudicate);
* at lambda2 = 0 x is not unique where the dictionary has no full column rank (more atoms than samples; SANDI's isotropic atoms): those
  runs are held to the certificate and to the error maps only -- and to what the certificate implies for A x, which IS unique: with
  g = A'(y - A x), |A (x - x')|^2 = (g' - g)'(x - x'), and two feasible points whose Kuhn-Tucker residuals are at most e = 1e-9 s make
  that at most 2 e (|x|_1 + |x'|_1) (AX_OF_KKT).  (The 1e-8 s the ridge-free cases of the small routes use would ask for more than the
  certificate does: a voxel that IS one atom has a zero residual at its optimum, every dual value is then of the size of the residual,
  and a mixture of the neighbouring zeppelins that meets every dual threshold to 1e-11 s leaves a residual of 1e-6 s.)
* error maps: |rmse - rmse_ld(device x)| <= 1e-9 rmse + 3e-8 rms(y), NRMSE likewise; SANDI's from the rescaled x against the normalised A;
* itercap_voxels == 0, overflow_voxels == 0; ctx.last_path() names k_enet_big;
* two more voxels, one with a NaN sample and one with +Inf in the last sample, give NaN maps and change no other voxel's bits.
"""
import os

import numpy as np
import pytest

import big_np as B
import czb_np as Z
import small_np as N

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
EPS = np.finfo(np.float64).eps


def _dev():
    import torch
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------ one fit of a case
def _upload(ctx, name):
    from amico_amd import _capi
    c, D = B.CASES[name], B.dictionary(name)
    ht = N._htable()['htable']
    if c['model'] == 'fw':
        return _capi.upload_freewater(ctx, D[0], ht)
    if c['model'] == 'sandi':
        return _capi.upload_sandi(ctx, D[0], D[1], D[2], D[3])
    return _capi.upload_czb(ctx, D[0], D[1], ht)


def _fit(ctx, L, name, lam, y, d, f32=None, **kw):
    """dict(est, rmse, nrmse, x [, yc, xiso]) of torch tensors: every output the route has"""
    import torch
    from amico_amd import _capi
    c = B.CASES[name]
    f32 = c['f32'] if f32 is None else f32
    yt = torch.from_numpy(np.array(y, dtype=np.float32 if f32 else np.float64)).to(_dev())
    dt = None if d is None else torch.from_numpy(np.array(d)).to(_dev())
    if c['model'] == 'fw':
        est, rmse, nrmse, yc, xd, xi = _capi.freewater_fit_device(ctx, L, yt, dt, lam[0], lam[1], c['mouse'], rmse=True, nrmse=True, corrected=True,
                                                                  return_x=True, iso=True, **kw)
        return dict(est=est, rmse=rmse, nrmse=nrmse, yc=yc, x=xd, xiso=xi)
    if c['model'] == 'sandi':
        est, rmse, nrmse, xd = _capi.sandi_fit_device(ctx, L, yt, lam[0], lam[1], rmse=True, nrmse=True, return_x=True, **kw)
    else:
        est, rmse, nrmse, xd = _capi.czb_fit_device(ctx, L, yt, dt, lam[0], lam[1], rmse=True, nrmse=True, return_x=True, **kw)
    return dict(est=est, rmse=rmse, nrmse=nrmse, x=xd)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _stats_clean(ctx, found):
    st = ctx.last_stats()
    if not (st['itercap_voxels'] == 0 and st['overflow_voxels'] == 0 and st['guard_trips'] == 0):
        found.append(('solver statistics', st))


def _with_bad_voxels(y):
    """two more voxels behind the others: copies of voxels 1 and 2 with a NaN sample / +Inf in the last sample"""
    bad = np.array(y[[1, 2]])
    bad[0, 3] = np.nan
    bad[1, -1] = np.inf
    return np.ascontiguousarray(np.vstack([y, bad]))


# ------------------------------------------------------------------------------------------------ the checks (test_gpu_small_hard.py's rule)
def _check(label, groups, y, kind, x, maps, maps_of_x, xo, mo, lam, n_atoms, unique=True, map_tol=1e-6):
    """x: the solver's coefficients of the device (SANDI: before the rescaling); maps_of_x(x) restates the maps from them.  unique=False
    (lambda2 = 0 without full column rank): the certificate and A x only.  Returns what it found wrong, one entry per property"""
    found = []
    lam1, lam2 = lam
    n = len(y)
    s = N.scale_of(y)
    if not (np.isfinite(x).all() and np.isfinite(maps).all()):
        return ['non-finite results on %d finite voxels' % int((~np.isfinite(x).all(axis=1) | ~np.isfinite(maps).all(axis=1)).sum())]
    ok, gps, gzs = np.zeros(n, bool), np.zeros(n), np.zeros(n)
    for rows, A in groups:
        ok[rows], gps[rows], gzs[rows] = N.kkt_ok(A, y[rows], x[rows], lam1, lam2)
    unit = Z.x_bound(n_atoms, lam2)
    by_x = unit <= 1e-6
    if not unique:
        ratio = np.zeros(n)
        for rows, A in groups:
            bound = np.sqrt(2.0 * N.KKT * s[rows] * (np.abs(x[rows]).sum(axis=1) + np.abs(xo[rows]).sum(axis=1)))      # AX_OF_KKT
            ratio[rows] = np.sqrt((((x[rows] - xo[rows]) @ A.T) ** 2).sum(axis=1)) / np.where(bound > 0, bound, 1.0)
    elif by_x:
        ratio = np.abs(x - xo).max(axis=1) / np.where(s > 0, unit * s, 1.0)
    else:
        thr = 1e-8 if lam2 == 0.0 else 1e-4
        ratio = np.zeros(n)
        for rows, A in groups:
            ratio[rows] = np.abs((x[rows] - xo[rows]) @ A.T).max(axis=1) / np.where(s[rows] > 0, thr * s[rows], 1.0)
    live = s > 0
    w = int(np.argmax(np.where(live, np.maximum(np.maximum(gps, gzs) / N.KKT, ratio), 0.0)))
    supp = (x > 0).sum(axis=1)
    print('BIGDICT %-30s gP/s %.2e  gZ/s %.2e  %s %.2e  worst: %s x %g  support mean %.0f max %d' %
          (label, gps[live].max(), gzs[live].max(), '|A dx|2/bound' if not unique else '|dx|/bound' if by_x else '|A dx|/bound', ratio.max(), N.KINDS[kind[w]], s[w], supp.mean(), supp.max()))
    if x[~live].any():
        found.append('an all-zero voxel with a non-zero x')
    if not ok.all():
        found.append(('certificate', 'voxels', int((~ok).sum()), 'first', int(np.flatnonzero(~ok)[0]), 'gP/s', float(gps.max()), 'gZ/s', float(gzs.max()),
                      'min x', float(x.min()), sorted(set(N.KINDS[k] for k in kind[~ok]))))
    if not (ratio <= 1.0).all():
        bad = ratio > 1.0
        found.append(('x against the oracle', 'voxels', int(bad.sum()), 'worst', float(ratio.max()), int(ratio.argmax()), sorted(set(N.KINDS[k] for k in kind[bad]))))
    # maps: the arithmetic alone
    mine = maps_of_x(x)
    tol = 1e-12 * np.abs(mine) + 1e-300
    if maps.shape[1] in (2, 4):
        tol[:, 1] += 4 * EPS
    err = np.abs(maps - mine) - tol
    if not (err <= 0.0).all():
        w = int(err.max(axis=1).argmax())
        found.append(('maps of the device x', 'voxels', int((err > 0).any(axis=1).sum()), w, maps[w].tolist(), mine[w].tolist()))
    if not unique:
        return found
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
    # maps against the oracle
    dm = N.map_distance(maps, mo)
    if not dm.max() < map_tol and lam2 > 0.0:
        dm = _adjudicate(groups, y, maps, mo, dm, xo, lam, maps_of_x, map_tol)
    if not dm.max() < map_tol:
        bad = ~(dm < map_tol)
        found.append(('maps against the oracle', 'voxels', int(bad.sum()), 'worst', float(dm.max()), int(dm.argmax()), sorted(set(N.KINDS[k] for k in kind[bad]))))
    return found


def _adjudicate(groups, y, maps, mo, dm, xo, lam, maps_of_solver_x, map_tol):
    """A voxel whose maps miss the oracle's by 1e-6 is taken to the long-double re-solve (czb_np.czb_resolve), the more exact of the two
    references: where the ORACLE's maps are off the re-solve's by more than 1e-8, the voxel's distance becomes that of the device maps
    from the re-solve's -- the bound stays what it was"""
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


def _check_errors(groups, y, x_err, rmse, nrmse):
    """x_err: the coefficients the error maps are made of (SANDI: the rescaled ones, against the normalised dictionary)"""
    rms = np.sqrt((y * y).mean(axis=1))
    found = []
    for rows, A in groups:
        ref = N.rmse_ld(A, y[rows], x_err[rows])
        bad = ~(np.abs(rmse[rows] - ref) <= 1e-9 * ref + 3e-8 * rms[rows])
        if bad.any():
            found.append(('rmse', 'voxels', int(bad.sum()), int(rows[bad][0]), float(rmse[rows][bad][0]), float(ref[bad][0]), float(rms[rows][bad][0])))
        ref = N.nrmse_ld(A, y[rows], x_err[rows])
        bad = ~(np.abs(nrmse[rows] - ref) <= 1e-9 * ref + 3e-8)
        if bad.any():
            found.append(('nrmse', 'voxels', int(bad.sum()), int(rows[bad][0]), float(nrmse[rows][bad][0]), float(ref[bad][0])))
    return found


def _same_bits(clean, dirty, n):
    """the run with the two bad voxels behind: NaN maps for them, every other voxel's outputs to the last bit what they were"""
    found = []
    for k in clean:
        a, b = clean[k], dirty[k]
        if k in ('est', 'rmse', 'nrmse', 'yc', 'xiso') and not np.isnan(b[n:]).all():
            found.append(('output of the bad voxels', k, b[n:].tolist()[:2]))
        if not np.array_equal(a, b[:n]):
            w = np.flatnonzero((a != b[:n]).reshape(n, -1).any(axis=1))
            found.append(('a bad voxel changed others', k, 'voxels', len(w), int(w[0])))
    return found


# ------------------------------------------------------------------------------------------------ 1. every shape, every voxel
@pytest.mark.parametrize('name,lam', B.BIG_RUNS, ids=B.ids(B.BIG_RUNS))
def test_big_dictionary_on_hard_voxels(name, lam):
    from amico_amd import get_context
    c = B.CASES[name]
    y, d, lut, kind = B.problem(name)
    xo, mo = B.reference(name, lam, NTHREADS)
    n, n_atoms = len(y), B.n_atoms_of(c)
    label = '%s (%g, %g)' % (name, lam[0], lam[1])
    ctx = get_context()
    L = _upload(ctx, name)
    found = []

    def fit(yy, dd):
        out = _fit(ctx, L, name, lam, yy, dd)
        ctx.sync()
        assert B.NEW_KERNEL in ctx.last_path(), (label, ctx.last_path())
        _stats_clean(ctx, found)
        return _host(out)
    clean = fit(y, d)
    dirty = fit(_with_bad_voxels(y), None if d is None else np.vstack([d, d[[1, 2]]]))
    L.close()
    found += _same_bits(clean, dirty, n)
    groups = B.groups(name)
    unique = not (lam[1] == 0.0)
    found += _check(label, groups, y, kind, B.solver_x(name, clean['x']), clean['est'], lambda x: B.maps_of(name, x), xo, mo, lam, n_atoms, unique=unique)
    found += _check_errors(groups, y, clean['x'], clean['rmse'], clean['nrmse'])
    if c['model'] == 'fw':
        n_perp, K = c['n_perp'], B.dictionary(name)[0]
        if not np.array_equal(clean['xiso'], clean['x'][:, n_perp:]):
            found.append('AMX_F_FW_ISO is not the last n_iso coefficients')
        ref = N.fw_corrected(y, clean['x'][:, n_perp:], K['CSF'].astype(np.float64))
        bad = ~(np.abs(clean['yc'] - ref) <= 8 * EPS * N.scale_of(y)[:, None]).all(axis=1)
        if bad.any():
            found.append(('corrected rows', 'voxels', int(bad.sum()), int(np.flatnonzero(bad)[0]), float(np.abs(clean['yc'] - ref).max())))
        assert (clean['yc'] == 0).any()
    assert not found, (label, found)


# ------------------------------------------------------------------------------------------------ 2. nothing changes at 64 atoms
@pytest.mark.parametrize('name,lam', B.SMALL_RUNS, ids=B.ids(B.SMALL_RUNS))
def test_64_atoms_take_none_of_the_new_kernels(name, lam):
    from amico_amd import get_context
    y, d, lut, kind = B.problem(name)
    xo, mo = B.reference(name, lam, NTHREADS)
    ctx = get_context()
    L = _upload(ctx, name)
    out = _fit(ctx, L, name, lam, y, d)
    ctx.sync()
    path = ctx.last_path()
    L.close()
    assert path and B.NEW_KERNEL not in path, path
    assert N.map_distance(out['est'].cpu().numpy(), mo).max() < 1e-6


def test_more_than_256_atoms_are_refused():
    from amico_amd import _capi, get_context, synthetic as S
    h = N._htable()
    sch = S.make_scheme(1, ((1000.0, 8),), seed=3)
    K = S.freewater_kernels(sch, h['dirs'], d_perps=np.linspace(0.05, 1.0, 256) * 1e-3)
    with pytest.raises(ValueError, match='n_atoms <= 256'):
        _capi.upload_freewater(get_context(), K, h['htable'])


# ------------------------------------------------------------------------------------------------ 3. bit-identity
@pytest.mark.parametrize('name', ['fw_33x101', 'sandi_6x65', 'czb_40x130'])
def test_float32_and_host_calls_are_bit_identical(name):
    """float32-rounded signals: the same bits through *_fit_device_f32 and *_fit_device; the host-buffer call gives them too"""
    from amico_amd import _capi, get_context
    c = B.CASES[name]
    lam = c['lams'][0]
    y, d, _, _ = B.problem(name)
    y32 = y.astype(np.float32)
    yw = y32.astype(np.float64)
    ctx = get_context()
    L = _upload(ctx, name)
    a = _fit(ctx, L, name, lam, yw, d, f32=False)
    ctx.sync()
    b = _fit(ctx, L, name, lam, y32, d, f32=True)
    ctx.sync()
    assert B.NEW_KERNEL in ctx.last_path()
    a, b = _host(a), _host(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (name, k)
    if c['model'] == 'fw':
        h = _capi.freewater_fit(ctx, L, yw, d, lam[0], lam[1], c['mouse'], rmse=True, nrmse=True, corrected=True)
        keys = ('est', 'rmse', 'nrmse', 'yc')
    elif c['model'] == 'sandi':
        h = _capi.sandi_fit(ctx, L, yw, lam[0], lam[1], rmse=True, nrmse=True)
        keys = ('est', 'rmse', 'nrmse')
    else:
        h = _capi.czb_fit(ctx, L, yw, d, lam[0], lam[1], rmse=True, nrmse=True)
        keys = ('est', 'rmse', 'nrmse')
    h32 = (_capi.sandi_fit(ctx, L, y32, lam[0], lam[1]) if c['model'] == 'sandi' else
           _capi.freewater_fit(ctx, L, y32, d, lam[0], lam[1], c['mouse']) if c['model'] == 'fw' else _capi.czb_fit(ctx, L, y32, d, lam[0], lam[1]))
    L.close()
    for k, v in zip(keys, h):
        assert np.array_equal(a[k], v), (name, 'host', k)
    assert np.array_equal(a['est'], h32[0]), (name, 'host float32')


# ------------------------------------------------------------------------------------------------ 4. amplitude
@pytest.mark.parametrize('name', ['fw_33x65', 'sandi_6x65', 'czb_40x65'])
def test_scale_equivariance(name):
    """signals times 2^-10 and 2^14 (lambda1 = 0): x and rmse are the unit-scale ones times c EXACTLY -- every threshold of the solver is
    relative to the voxel, and a power of two commutes with every rounding --, nrmse bit for bit, the maps the unit-scale maps up to their
    1e-16 guards (1e-9 on the voxels whose coefficients sum to more than 1e-4 at unit scale: 1e-16 / (2^-10 1e-4))"""
    from amico_amd import get_context
    c = B.CASES[name]
    lam = c['lams'][0]
    assert lam[0] == 0.0
    y, d, _, _ = B.problem(name)
    s = N.scale_of(y)
    unit = np.flatnonzero((s == 0) | ((s > 2.0 ** -6) & (s < 2.0 ** 6)))      # (hard_mix: the voxels it left at amplitude 1 -- the others pass nrmse's
    #                                                                            absolute guard sum y^2 > 1e-16 at one scale and not at the other)
    y, d = y[unit], None if d is None else d[unit]
    ctx = get_context()
    L = _upload(ctx, name)
    one = _fit(ctx, L, name, lam, y, d, f32=False)
    ctx.sync()
    one = _host(one)
    for cs in (2.0 ** -10, 2.0 ** 14):
        got = _fit(ctx, L, name, lam, y * cs, d, f32=False)
        ctx.sync()
        st = ctx.last_stats()
        assert st['itercap_voxels'] == 0 and st['guard_trips'] == 0, st
        got = _host(got)
        assert np.array_equal(got['x'], one['x'] * cs), (name, cs, float(np.abs(got['x'] / cs - one['x']).max()))
        assert np.array_equal(got['rmse'], one['rmse'] * cs), (name, cs)
        assert np.array_equal(got['nrmse'], one['nrmse']), (name, cs)
        solid = one['x'].sum(axis=1) > 1e-4
        assert np.isfinite(got['est']).all()
        assert N.map_distance(got['est'][solid], one['est'][solid]).max() <= 1e-9, (name, cs)
    L.close()


# ------------------------------------------------------------------------------------------------ 5. bad directions
@pytest.mark.parametrize('name', ['fw_33x65', 'czb_40x65'])
def test_a_nan_direction_names_its_voxel_and_disturbs_nobody(name):
    """a 200-voxel call with one NaN direction, behind a larger call on the same context (whose bucketed order is still in the workspace):
    RuntimeError naming the voxel, its row zero, and every other row to the last bit what the call without the bad direction gives -- the
    kernel walks the bucketed count on the device, not n"""
    from amico_amd import get_context
    lam = B.CASES[name]['lams'][0]
    y, d, _, _ = B.problem(name)
    ctx = get_context()
    L = _upload(ctx, name)
    _fit(ctx, L, name, lam, y, d)
    ctx.sync()
    y2, d2 = y[:200], np.array(d[:200])
    good = _fit(ctx, L, name, lam, y2, d2)
    ctx.sync()
    d2[137] = np.nan
    out = _fit(ctx, L, name, lam, y2, d2)
    with pytest.raises(RuntimeError, match=r'index out of bounds.*\[voxel 137\]'):
        ctx.sync()
    assert B.NEW_KERNEL in ctx.last_path()
    good, out = _host(good), _host(out)
    L.close()
    others = np.arange(200) != 137
    assert (out['est'][137] == 0.0).all() and (out['x'][137] == 0.0).all()
    for k in ('est', 'rmse', 'nrmse', 'x'):
        assert np.array_equal(out[k][others], good[k][others]), (name, k)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_evaluation_freewater_with_80_d_perps(htable500):
    """set_model -> model.set(80 d_perps) -> generate_kernels -> load_kernels -> fit() on a 12 x 12 x 4 image over a small direction set,
    with doSaveCorrectedDWI, doSavePredictedSignal and doComputeNRMSE: RESULTS against model.fit on the downloaded y and DIRs"""
    import amico_amd
    from amico_amd import synthetic as S
    lut_dirs = htable500['dirs']
    rng = np.random.default_rng(11)
    sch = S.make_scheme(1, ((1000.0, 32),), seed=3)
    shape = (12, 12, 4)
    n = int(np.prod(shape))
    mask = np.ones(shape, dtype=np.uint8)
    d_perps = np.linspace(0.05, 1.0, 80) * 1e-3

    def evaluation(img, peaks):
        ae = amico_amd.Evaluation()
        for k in ('doSaveCorrectedDWI', 'doSavePredictedSignal', 'doComputeNRMSE'):
            ae.set_config(k, True)
        ae.set_data(img, sch, mask, peaks)
        ae.set_model('FreeWater')
        ae.model.set(d_perps=d_perps)
        return ae
    ae = evaluation(np.ones(shape + (sch.nS,), dtype=np.float32), None)
    ae.load_kernels(ae.generate_kernels(lut_dirs), lut_dirs)
    K = ae.KERNELS
    assert K['D'].shape == (80, len(lut_dirs), sch.nS) and K['CSF'].shape == (1, sch.nS)
    ori = rng.choice(np.array([17, 203, 431, 44, 310]), n)           # a small direction set
    atom, fw = rng.integers(0, 80, n), rng.uniform(0.1, 0.6, n)
    y = (1.0 - fw)[:, None] * K['D'][atom, ori].astype(np.float64) + fw[:, None] * K['CSF'][0][None, :].astype(np.float64)
    y = np.abs(y + rng.normal(scale=0.02, size=y.shape))
    img = (1000.0 * y).reshape(shape + (sch.nS,)).astype(np.float32)
    ae2 = evaluation(img, lut_dirs[ori].reshape(shape + (3,)))
    ae2.set_kernels(K, ae.htable)
    res = ae2.fit()
    assert list(res) == ['estimates', 'nrmse', 'y_corrected', 'y_est']
    R = ae2.RESULTS
    assert R['MAPs'].shape == shape + (2,) and R['DWI_corrected'].shape == img.shape and R['DWI_predicted'].shape == img.shape

    class Holder:
        y, DIRs, htable, KERNELS, nthreads = ae2.y, ae2.DIRs, ae2.htable, K, 4

        def get_config(self, k):
            return ae2.get_config(k) if k in ('doMergeB0', 'doDirectionalAverage', 'solver_params', 'doComputeNRMSE', 'doSaveCorrectedDWI') else False
    own = ae2.model.fit(Holder())                                       # numpy in / numpy out: the host-buffer call
    assert np.array_equal(R['MAPs'].reshape(n, 2), own['estimates'].astype(np.float32))
    assert np.array_equal(R['NRMSE'].reshape(n), own['nrmse'].astype(np.float32))
    assert np.array_equal(res['y_corrected'], own['y_corrected'])
    mb0 = ae2.mean_b0s.reshape(n, 1)
    assert np.abs(R['DWI_corrected'].reshape(n, -1) - own['y_corrected'] * mb0).max() <= 1e-6 * np.abs(img).max()
    # the prediction is A x: its residual is the error map, and the corrected rows are the prediction without its isotropic part where unclipped
    assert np.abs(np.sqrt(((ae2.y - res['y_est']) ** 2).sum(axis=1) / (ae2.y ** 2).sum(axis=1)) - res['nrmse']).max() < 1e-6
    assert np.abs(R['DWI_predicted'].reshape(n, -1) - res['y_est'] * mb0).max() <= 1e-6 * np.abs(img).max()
    # and the maps are the oracle's
    from oracle import oracle
    ref = oracle.freewater_fit(ae2.y, ae2.DIRs, K, ae2.htable, nthreads=NTHREADS)['estimates']
    assert np.abs(R['MAPs'].reshape(n, 2) - ref.astype(np.float32)).max() < 1e-5
