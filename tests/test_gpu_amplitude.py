"""Every fit path at signal amplitudes far from one.

The reference accepts signals of any amplitude: `b0_min_signal = 0` (core.py set_data) divides by any positive mean b0, so a voxel
at the brain's edge reaches the fit at 10^2 - 10^4, and `doNormalizeSignal = False` hands raw intensities to every model.  The
device solvers make many decisions against absolute constants (stop tests, certificate margins, the Gram / exact dual switch),
tuned on unit-amplitude data.

The exact reference needs no tolerance tuning: scale equivariance.  For c > 0, NNLS gives x(c y) = c x(y) and the non-negative
elastic net with (c lambda1, lambda2) gives c x (pinned for the oracle in test_oracle.py), so every map is invariant and RMSE,
the corrected DWI and the coefficients scale by c.  The unit-scale device fit -- itself pinned by the oracle and by the KKT
certificates of test_gpu_kkt.py -- is therefore the reference at every scale.  Powers of two with even exponents keep c y exact
in float32 and float64.

Then the two reference configs end to end through Evaluation, against the numpy signal preparation plus the oracle fits:
raw intensities (doNormalizeSignal = False) and the default normalisation with some voxels of a tiny mean b0.
"""
import os

import numpy as np
import pytest

from kkt_certificates import by_direction, noddi_certificates

pytestmark = pytest.mark.gpu

SCALES = (2.0 ** -10, 2.0 ** -4, 2.0 ** 4, 2.0 ** 10, 2.0 ** 14)
N_VOX = 100_000
CAP = 1e-4            # BASELINE.json: maps within 1e-4 of the reference on EVERY voxel
NEAR = 1e-6           # ... and at least 99.99 % of the voxels within 1e-6 (the standard of test_gpu_kkt.py)
SCALED_REL = 1e-9     # RMSE, corrected DWI: c times the unit-scale value, relative
NTHREADS = min(16, os.cpu_count() or 1)


def _dev():
    import torch
    return torch.device('cuda', 0)


def _compare_maps(label, c, maps, ref):
    """maps [n, k] at scale c against the unit-scale device maps: printed (the table of the PR) and held to CAP / NEAR"""
    diff = np.abs(maps - ref).max(axis=1)
    bitwise = float(np.all(maps == ref, axis=1).mean())
    print('AMPLITUDE %-40s c = 2^%-3d  max %.3e  > 1e-6: %5d  bitwise equal %.4f'
          % (label, int(np.log2(c)), diff.max(), int((diff > NEAR).sum()), bitwise))
    assert np.isfinite(maps).all(), (label, c)
    assert diff.max() <= CAP, (label, c, float(diff.max()), int(diff.argmax()))
    assert (diff <= NEAR).mean() >= 0.9999, (label, c, int((diff > NEAR).sum()))


def _compare_scaled(label, c, v, v1, y1):
    """a quantity that scales with the signal (RMSE [n], corrected DWI [n, nS]): v = c v1 to SCALED_REL of the voxel's own value,
    plus 3e-8 of the RMS of its unit-scale signal y1.  (That floor is the RMSE of the seeded NODDI chain, which comes from the Gram
    form ||y||^2 - z'c: on a voxel the dictionary explains exactly -- a flat one ex vivo, true RMSE 0 -- it is rounding noise of
    ||y||^2 under a square root, up to sqrt(4 eps) ~ 2e-8 of the signal's RMS, and not a value that scales with c.)"""
    v, v1 = v.reshape(len(v), -1), v1.reshape(len(v1), -1)
    err = np.abs(v / c - v1).max(axis=1)
    tol = SCALED_REL * np.abs(v1).max(axis=1) + 3e-8 * np.sqrt((y1 * y1).mean(axis=1))
    bad = err > tol
    assert not bad.any(), (label, c, float((err[bad] / tol[bad]).max()), int(bad.sum()))


def _stats_clean(ctx, label):
    st = ctx.last_stats()
    assert st['itercap_voxels'] == 0 and st['guard_trips'] == 0 and st['overflow_voxels'] == 0, (label, st)


# ------------------------------------------------------------------------------------------------------------- NODDI
def _noddi_fit(ctx, lut, y, d, lam1, lam2, n_maps):
    import torch
    from amico_amd import _capi
    yt, dt = torch.from_numpy(y).to(_dev()), torch.from_numpy(d).to(_dev())
    est, r, nr, md, xd = _capi.noddi_fit_device(ctx, lut, yt, dt, lam1, lam2, n_maps, rmse=True, nrmse=True, mod=True,
                                                return_x=True)
    ctx.sync()
    return {'maps': np.concatenate([est.cpu().numpy(), md.cpu().numpy(), nr.cpu().numpy()[:, None]], axis=1),
            'rmse': r.cpu().numpy(), 'x': xd.cpu().numpy(), 'path': ctx.last_path(), 'seed': ctx.last_seed_stats()}


NODDI_CASES = {
    # id: (signals, ex vivo, number of voxels, lambda1, switches, expected mapping)
    'clean seeded':             ('clean', False, N_VOX, 0.5, {}, 'seeded'),
    'hard seeded':              ('hard', False, N_VOX, 0.5, {}, 'seeded'),
    'hard seeded ex vivo':      ('hard', True, N_VOX, 0.5, {}, 'seeded'),
    'hard rescue pass':         ('hard', False, N_VOX, 0.5, {'AMX_RESCUE_FROM': '0'}, 'seeded'),
    'hard tight trip caps':     ('hard', False, N_VOX, 0.5, {'AMX_SEED_TRIPCAP': '6,5,4'}, 'seeded'),
    'clean wavefront':          ('clean', False, 15_000, 0.5, {}, 'wave'),
    'hard wavefront ex vivo':   ('hard', True, 15_000, 0.5, {}, 'wave'),
    'clean no seed':            ('clean', False, N_VOX, 0.5, {'AMX_NO_SEED': '1'}, 'wave'),
    'clean lambda1 = 0':        ('clean', False, 20_000, 0.0, {}, 'big'),
}


@pytest.mark.parametrize('case', list(NODDI_CASES))
def test_noddi_is_scale_equivariant_on_every_path(htable500, case, amx_env):
    """maps (NDI / ODI / FWF, ex vivo fraction, modulated maps, NRMSE) invariant, RMSE scaling with c, the KKT certificates of the
    device x with their tolerances times c, no capped / guarded / overflowing voxel and the same kernels at every scale"""
    from amico_amd import _capi, get_context, synthetic as S
    kind, exvivo, n, lam1, env, mapping = NODDI_CASES[case]
    if env:
        amx_env(**env)
    lam2, n_maps = 1e-3, 4 if exvivo else 3
    dirs, ht = htable500['dirs'], htable500['htable']
    sch = S.make_scheme(seed=9 if kind == 'hard' else 0)
    K = S.noddi_kernels(sch, dirs)
    if kind == 'hard':
        y, d, _ = S.noddi_hard_signals(n, K, ht, sch, seed=19)
        tol = 4e-9                                       # test_gpu_kkt.py: the hard mix's bound at unit amplitude
    else:
        y, d = S.noddi_signals(n, K, ht, sch, seed=31, snr=30.0)
        tol = 1e-9
    ctx = get_context()
    lut = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx, is_exvivo=exvivo)
    ref = _noddi_fit(ctx, lut, y, d, lam1, lam2, n_maps)
    _stats_clean(ctx, case)
    if mapping == 'seeded':
        assert ref['seed']['seeded_voxels'] == n, ref['seed']
    elif mapping == 'wave':
        assert ref['seed']['seeded_voxels'] == 0, ref['seed']
    else:
        assert 'k_noddi_lasso_big' in ref['path'], ref['path']
    for c in (1.0,) + SCALES:
        out = ref if c == 1.0 else _noddi_fit(ctx, lut, c * y, d, lam1 * c, lam2, n_maps)
        _stats_clean(ctx, (case, c))
        assert out['path'] == ref['path'], (case, c, out['path'], ref['path'])      # amplitude must not change the kernels that run
        assert out['seed']['seeded_voxels'] == ref['seed']['seeded_voxels'], (case, c)
        if c != 1.0:
            _compare_maps('NODDI ' + case, c, out['maps'], ref['maps'])
            _compare_scaled('NODDI ' + case, c, out['rmse'], ref['rmse'], y)
        cert = noddi_certificates(K, sch, ht, c * y, d, out['x'], lam1 * c, lam2, exvivo=exvivo)
        assert cert['min_x'] >= 0.0 and cert['s3_off_support'] == 0.0, (case, c, cert)
        assert max(cert['s1_wP'], cert['s2_gP'], cert['s3_wP']) < tol * c, (case, c, cert)
        assert max(cert['s1_wZ'], cert['s2_gZ'], cert['s3_wZ']) < tol * c, (case, c, cert)


# ------------------------------------------------------------------------------------------------------------- FreeWater
def _lasso_certificate(A, Y, X, lam1, lam2):
    G = (Y - X @ A.T) @ A - lam2 * X - lam1
    P = X > 0
    return float(np.abs(G[P]).max(initial=0.0)), float(G[~P].max(initial=0.0)), float(X.min())


@pytest.mark.parametrize('mapping,is_mouse', [('refill', False), ('refill', True), ('lane', False), ('wave', True)])
def test_freewater_is_scale_equivariant(htable500, mapping, is_mouse, amx_env):
    """mapping as in test_freewater_kkt_certificates: 'refill' (default), 'lane' (AMX_NO_REFILL), 'wave' (AMX_WAVE_PER_VOXEL)"""
    import torch
    from amico_amd import _capi, get_context, synthetic as S
    if mapping == 'wave':
        amx_env(AMX_WAVE_PER_VOXEL='1')
    if mapping == 'lane':
        amx_env(AMX_NO_REFILL='1')
    n = 20_000 if mapping == 'wave' else N_VOX
    dirs, ht = htable500['dirs'], htable500['htable']
    sch = S.make_scheme(1, ((1000.0, 64),), seed=3)
    K = S.freewater_kernels(sch, dirs, d_isos=(2.0e-3, 3.0e-3) if is_mouse else (2.5e-3,))       # (Mouse: two isotropic atoms)
    y, d = S.freewater_signals(n, K, ht, sch, seed=17, snr=10.0)
    ctx = get_context()
    lut = _capi.upload_freewater(ctx, K, ht)
    dt = torch.from_numpy(d).to(_dev())
    idx = S.lut_indices(d, ht)
    groups = by_direction(idx)
    label = 'FreeWater %s%s' % (mapping, ' mouse' if is_mouse else '')
    ref = None
    for c in (1.0,) + SCALES:
        est, r, nr, yc, xd = _capi.freewater_fit_device(ctx, lut, torch.from_numpy(c * y).to(_dev()), dt, 0.0, 1e-3, is_mouse,
                                                        rmse=True, nrmse=True, corrected=True, return_x=True)
        ctx.sync()
        _stats_clean(ctx, (label, c))
        out = {'maps': np.concatenate([est.cpu().numpy(), nr.cpu().numpy()[:, None]], axis=1), 'rmse': r.cpu().numpy(),
               'yc': yc.cpu().numpy(), 'path': ctx.last_path()}
        x = xd.cpu().numpy()
        gp = gz = 0.0
        for rows in groups:
            A = np.concatenate([K['D'][:, idx[rows[0]], :], K['CSF']], axis=0).astype(np.float64).T
            a, b, mn = _lasso_certificate(A, c * y[rows], x[rows], 0.0, 1e-3)
            gp, gz = max(gp, a), max(gz, b)
            assert mn >= 0.0
        assert gp < 1e-9 * c and gz < 1e-9 * c, (label, c, gp, gz)
        if ref is None:
            ref = out
            continue
        assert out['path'] == ref['path'], (label, c, out['path'], ref['path'])
        _compare_maps(label, c, out['maps'], ref['maps'])
        _compare_scaled(label, c, out['rmse'], ref['rmse'], y)
        _compare_scaled(label + ' corrected DWI', c, out['yc'], ref['yc'], y)


# ------------------------------------------------------------------------------------------------------------- SANDI
@pytest.mark.parametrize('mapping', ['rows', 'lane', 'wave'])
def test_sandi_is_scale_equivariant(mapping, amx_env):
    import torch
    from amico_amd import _capi, get_context, synthetic as S
    if mapping == 'wave':
        amx_env(AMX_WAVE_PER_VOXEL='1')
    if mapping == 'lane':
        amx_env(AMX_SANDI_ATOM_SPACE='1')
    n = N_VOX if mapping == 'rows' else 20_000
    avg = S.directional_average_scheme(S.make_sandi_scheme())
    K, Rs, d_in, d_isos = S.sandi_kernels(avg)
    y = S.sandi_signals(n, K, avg, seed=23, snr=10.0)
    ctx = get_context()
    lut = _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)
    A = np.asarray(K['signal'], dtype=np.float64)
    label = 'SANDI ' + mapping
    ref = None
    for c in (1.0,) + SCALES:
        est, r, nr, xd = _capi.sandi_fit_device(ctx, lut, torch.from_numpy(c * y).to(_dev()), 0.0, 5e-3, rmse=True, nrmse=True,
                                                return_x=True)
        ctx.sync()
        _stats_clean(ctx, (label, c))
        e = est.cpu().numpy()
        out = {'fractions': np.concatenate([e[:, :3], nr.cpu().numpy()[:, None]], axis=1), 'sizes': e[:, 3:],
               'rmse': r.cpu().numpy(), 'path': ctx.last_path()}
        x = xd.cpu().numpy() / K['norms'][None, :]               # undo models.pyx:1570-1571 for the certificate
        gp, gz, mn = _lasso_certificate(A, c * y, x, 0.0, 5e-3)
        assert mn >= 0.0 and gp < 1e-9 * c and gz < 1e-9 * c, (label, c, gp, gz, mn)
        if ref is None:
            ref = out
            continue
        assert out['path'] == ref['path'], (label, c, out['path'], ref['path'])
        _compare_maps(label, c, out['fractions'], ref['fractions'])
        # Rsoma / Din / De (um, um^2/ms): relative, as test_sandi_kkt_certificates compares them
        den = np.abs(ref['sizes']) + 1e-3
        _compare_maps(label + ' sizes (rel)', c, out['sizes'] / den, ref['sizes'] / den)
        _compare_scaled(label, c, out['rmse'], ref['rmse'], y)


# ------------------------------------------------------------------------------------------------------------- CylinderZeppelinBall
def test_czb_is_scale_equivariant(czb_fix, htable500):
    import torch
    from amico_amd import _capi, get_context, synthetic as S
    f = czb_fix
    ht, K, ids = htable500['htable'], f['kernels'], f['lut_ids']
    rng = np.random.default_rng(13)
    dirs = []
    while sum(len(d) for d in dirs) < 20000:                        # directions in the LUT cells the fixture has dictionaries for
        dd = S.random_unit_vectors(400000, rng)
        dirs.append(dd[np.isin(S.lut_indices(dd, ht), ids)])
    d = np.concatenate(dirs)[:20000]
    lut_i = S.lut_indices(d, ht)
    n = len(d)
    n_rs, n_p = K['wmr'].shape[0], K['wmh'].shape[0]
    w = rng.dirichlet([2.0, 2.0, 1.0], n)
    y0 = w[:, :1] * K['wmr'][rng.integers(n_rs, size=n), lut_i].astype(np.float64) + \
        w[:, 1:2] * K['wmh'][rng.integers(n_p, size=n), lut_i].astype(np.float64) + w[:, 2:] * K['iso'][0].astype(np.float64)
    y = np.abs(y0 + rng.normal(scale=1 / 20.0, size=y0.shape) + 1j * rng.normal(scale=1 / 20.0, size=y0.shape))
    y = y.astype(np.float32).astype(np.float64)
    ctx = get_context()
    L = _capi.upload_czb(ctx, K, f['Rs'], ht)
    dt = torch.from_numpy(d).to(_dev())
    ref = None
    for c in (1.0,) + SCALES:
        est, r, nr, xd = _capi.czb_fit_device(ctx, L, torch.from_numpy(c * y).to(_dev()), dt, 0.0, 4.0, rmse=True, nrmse=True,
                                              return_x=True)
        ctx.sync()
        _stats_clean(ctx, ('CZB', c))
        out = {'maps': est.cpu().numpy(), 'nrmse': nr.cpu().numpy()[:, None], 'rmse': r.cpu().numpy(), 'path': ctx.last_path()}
        x = xd.cpu().numpy()
        gp = gz = 0.0
        for lid in ids:
            rows = np.flatnonzero(lut_i == lid)
            A = np.concatenate([K['wmr'][:, lid], K['wmh'][:, lid], K['iso']], axis=0).astype(np.float64).T
            a, b, mn = _lasso_certificate(A, c * y[rows], x[rows], 0.0, 4.0)
            gp, gz = max(gp, a), max(gz, b)
            assert mn >= 0.0
        assert gp < 1e-9 * c and gz < 1e-9 * c, ('CZB', c, gp, gz)
        if ref is None:
            ref = out
            continue
        assert out['path'] == ref['path'], ('CZB', c, out['path'], ref['path'])
        # v / a / d relative to the unit-scale maps, as test_gpu_czb.py compares them
        den = np.abs(ref['maps']) + 1e-3
        _compare_maps('CylinderZeppelinBall v/a/d (rel)', c, out['maps'] / den, ref['maps'] / den)
        _compare_maps('CylinderZeppelinBall NRMSE', c, out['nrmse'], ref['nrmse'])
        _compare_scaled('CylinderZeppelinBall', c, out['rmse'], ref['rmse'], y)


# ------------------------------------------------------------------------------------------------------------- batched solvers
def _dictionaries(shape, htable500):
    """[n_dicts, m, n] with unit columns: (99, 145) the NODDI stage-1 dictionaries, (6, 15) SANDI's, otherwise random positive ones.
    (200, 60) is the NR = 4 build with the tile in LDS, (300, 200) and (512, 256) take the global-tile path."""
    from amico_amd import synthetic as S
    m, n = shape
    if shape == (99, 145):
        sch = S.make_scheme(seed=0)
        K = S.noddi_kernels(sch, htable500['dirs'])
        A = np.stack([np.concatenate([K['wm'][:, dd, :].astype(np.float64), K['iso'][None, :].astype(np.float64)], axis=0).T
                      for dd in range(0, 500, 84)])
    elif shape == (6, 15):
        avg = S.directional_average_scheme(S.make_sandi_scheme())
        A = np.asarray(S.sandi_kernels(avg)[0]['signal'], dtype=np.float64)[None]
    else:
        rng = np.random.default_rng(m + n)
        A = np.abs(rng.normal(size=(3, m, n))) + 0.1 * rng.random((3, m, n))
    return A / np.linalg.norm(A, axis=1, keepdims=True)


def _nnls_kkt(A, y, x):
    W = A.T @ (y - A @ x)
    return float(np.abs(W[x > 0]).max(initial=0.0)), float(W[x == 0].max(initial=0.0))


def _enet_kkt(A, y, x, lam1, lam2):
    g = A.T @ (y - A @ x) - lam2 * x - lam1
    return float(np.abs(g[x > 0]).max(initial=0.0)), float(g[x == 0].max(initial=0.0))


def _batched_at_every_scale(label, A, y, idx, lam1, lam2, sample):
    """nnls_batched / lasso_batched at every scale: x >= 0, the Kuhn-Tucker conditions with tolerances times c, scipy's NNLS on
    every `sample`-th voxel, and the fit against the unit-scale device fit"""
    from scipy.optimize import nnls as scipy_nnls
    from amico_amd import _capi, get_context
    from oracle import oracle
    ctx = get_context()
    dic = _capi.Dict(ctx, A)
    nv = len(y)
    ref = None
    for c in (1.0,) + SCALES:
        x, rn = _capi.nnls_batched(ctx, dic, c * y, idx, return_rnorm=True)
        _stats_clean(ctx, (label, 'nnls', c))
        xl = _capi.lasso_batched(ctx, dic, c * y, lam1 * c, lam2, idx)
        _stats_clean(ctx, (label, 'lasso', c))
        assert x.min() >= 0.0 and xl.min() >= 0.0
        for v in range(nv):
            Av = A[idx[v]]
            wp, wz = _nnls_kkt(Av, c * y[v], x[v])
            assert wp < 1e-9 * c and wz < 1e-9 * c, (label, 'nnls', c, v, wp, wz)
            gp, gz = _enet_kkt(Av, c * y[v], xl[v], lam1 * c, lam2)
            assert gp < 1e-9 * c and gz < 1e-9 * c, (label, 'lasso', c, v, gp, gz)
            if v % sample == 0:
                # Lawson-Hanson (the oracle's restatement), and scipy's where m >= n (its NNLS can stop short of the optimum on
                # underdetermined problems: a positive dual value off its support of ~1e-6 on the 6 x 15 SANDI dictionary)
                refs = [oracle.nnls(Av, c * y[v])[:2]] + ([scipy_nnls(Av, c * y[v], maxiter=50 * Av.shape[1])] if Av.shape[0] >= Av.shape[1] else [])
                for xs, rs in refs:
                    assert abs(rn[v] - rs) < 1e-9 * c and np.abs(Av @ (x[v] - xs)).max() < 1e-8 * c, (label, c, v, rn[v], rs)
        if ref is None:
            ref = (x, xl)
            continue
        _compare_maps(label + ' nnls A x / c', c, np.einsum('vmn,vn->vm', A[idx], x / c), np.einsum('vmn,vn->vm', A[idx], ref[0]))
        _compare_maps(label + ' lasso x / c', c, xl / c, ref[1])    # strictly convex (lambda2 > 0): x itself is unique
    return ref


@pytest.mark.parametrize('shape', [(99, 145), (6, 15), (200, 60), (300, 200), (512, 256)])
def test_batched_solvers_are_scale_equivariant(htable500, shape):
    A = _dictionaries(shape, htable500)
    nd, m, n = A.shape
    rng = np.random.default_rng(7 + m)
    nv = 600
    idx = rng.integers(0, nd, nv).astype(np.int32)
    k = min(4, n)
    cols = np.stack([rng.choice(n, k, replace=False) for _ in range(nv)])
    w = rng.dirichlet(np.ones(k), nv)
    y = np.stack([A[idx[v]][:, cols[v]] @ w[v] for v in range(nv)])
    y = np.abs(y + rng.normal(scale=0.003, size=y.shape))
    y[3] = 0.0                                                          # all-zero signal: x = 0
    _batched_at_every_scale('batched %dx%d' % shape, A, y, idx, 0.1, 1e-3, 10)


def _support_problem(m, n, sizes, rng):
    """dictionary [m, n] with m > n and signals whose NNLS optimum is a given support P of k atoms: y = A_P x_P + r, x_P in
    [0.5, 1.5], with a residual r (2 % of the signal: a little noise the optimum cannot absorb) orthogonal to the support's columns
    and with A_j' r equal and negative for every other atom -- then x_P is the NNLS solution itself, with a strict margin"""
    A = np.abs(rng.normal(size=(m, n))) + 0.2
    A /= np.linalg.norm(A, axis=0, keepdims=True)
    ys, xs = [], []
    for k in sizes:
        P = np.sort(rng.choice(n, k, replace=False))
        Z = np.setdiff1d(np.arange(n), P)
        x = np.zeros(n)
        x[P] = rng.uniform(0.5, 1.5, k)
        Q, _ = np.linalg.qr(A[:, P])
        B = A[:, Z] - Q @ (Q.T @ A[:, Z])                             # the other atoms off the support's span
        r = -B @ np.linalg.solve(B.T @ B, np.ones(len(Z)))             # A_Z' r = -1, A_P' r = 0
        y = A @ x + 0.02 * np.linalg.norm(A @ x) * r / np.linalg.norm(r)
        ys.append(y)
        xs.append(x)
    return A, np.array(ys), np.array(xs)


@pytest.mark.parametrize('m,n', [(200, 60), (120, 56), (300, 64)])
def test_batched_solvers_supports_of_17_to_48_atoms(m, n):
    """optimal supports of 20 - 48 atoms: beyond the main pass's 16, in the one-wavefront re-run pass (MB = 48) -- with the tile in
    LDS for NR = 4 (200 x 60) and NR = 2 (120 x 56), and on the global-tile path (300 x 64)"""
    from scipy.optimize import nnls as scipy_nnls
    rng = np.random.default_rng(m * n)
    sizes = np.repeat(np.arange(20, 49), 4)
    A, y, xt = _support_problem(m, n, sizes, rng)
    for v in range(len(y)):                                           # confirm the supports in numpy (scipy's Lawson-Hanson)
        xs, _ = scipy_nnls(A, y[v], maxiter=50 * n)
        assert (xs > 0).sum() == sizes[v] and np.abs(xs - xt[v]).max() < 1e-9
    idx = np.zeros(len(y), dtype=np.int32)
    x, xl = _batched_at_every_scale('supports 20-48 %dx%d' % (m, n), A[None], y, idx, 1e-4, 1e-4, 3)
    assert np.array_equal((x > 0).sum(axis=1), sizes) and np.abs(x - xt).max() < 1e-9
    assert ((xl > 0).sum(axis=1) == sizes).all()


def test_batched_solvers_refuse_a_49_atom_optimum():
    """a 49-atom optimum is beyond the passive set (48): AMX_E_OVERFLOW at every scale, never a wrong x"""
    from scipy.optimize import nnls as scipy_nnls
    from amico_amd import _capi, get_context
    rng = np.random.default_rng(49)
    A, y, xt = _support_problem(200, 60, [49] * 8, rng)
    assert all((scipy_nnls(A, yy, maxiter=3000)[0] > 0).sum() == 49 for yy in y)
    ctx = get_context()
    dic = _capi.Dict(ctx, A)
    for c in (1.0,) + SCALES:
        with pytest.raises(_capi.AmxError) as e:
            _capi.nnls_batched(ctx, dic, c * y)
        assert e.value.code == _capi.AMX_E_OVERFLOW, (c, e.value)
        with pytest.raises(_capi.AmxError) as e:
            _capi.lasso_batched(ctx, dic, c * y, 1e-4 * c, 1e-4)
        assert e.value.code == _capi.AMX_E_OVERFLOW, (c, e.value)


# ------------------------------------------------------------------------------------------------------------- the reference's configs end to end
def _volume_case(model, htable500, config):
    """(image, scheme, mask, peaks, kernels): NODDI on a 32^3 volume (31 000 masked voxels: the seeded chain), FreeWater on 24 x 24 x 16.
    config 'raw': b0 ~ 1000 and no normalisation; 'tiny b0': 2 % of the masked voxels have a mean b0 of 1e-4 - 1e-1 of the tissue's
    (after the default normalisation, b0_min_signal = 0, their diffusion-weighted volumes reach ~10^4)"""
    from amico_amd import synthetic as S
    ht = htable500['htable']
    rng = np.random.default_rng(61 if model == 'NODDI' else 62)
    if model == 'NODDI':
        sch = S.make_scheme(seed=0)
        K = S.noddi_kernels(sch, htable500['dirs'])
        shape = (32, 32, 32)
        y, d = S.noddi_signals(int(np.prod(shape)), K, ht, sch, seed=63)
    else:
        sch = S.make_scheme(2, ((1000.0, 64),), seed=3)
        K = S.freewater_kernels(sch, htable500['dirs'])
        shape = (24, 24, 16)
        y, d = S.freewater_signals(int(np.prod(shape)), K, ht, sch, seed=64)
    img = y.reshape(shape + (-1,)) * 1000.0 * rng.uniform(0.8, 1.2, shape)[..., None]
    mask = (rng.uniform(size=shape) < 0.95).astype(np.uint8)
    if config == 'tiny b0':
        sel = np.flatnonzero((mask.ravel() == 1) & (rng.uniform(size=mask.size) < 0.02))
        flat = img.reshape(-1, img.shape[-1])
        f = 10.0 ** rng.uniform(-4.0, -1.0, len(sel))
        flat[np.ix_(sel, np.asarray(sch.b0_idx))] *= f[:, None]
    return img.astype(np.float32), sch, mask, d.reshape(shape + (3,)), K


@pytest.mark.parametrize('config', ['raw', 'tiny b0'])
@pytest.mark.parametrize('model', ['NODDI', 'FreeWater'])
def test_reference_configs_end_to_end(htable500, model, config):
    """Evaluation (doNormalizeSignal = False on raw intensities with the default lambdas; or the default normalisation with tiny
    b0s) against oracle/signal_np.prepare_signal plus the oracle fit: every voxel within 1e-4"""
    import amico_amd
    from oracle import oracle, signal_np
    ht = htable500['htable']
    img, sch, mask, peaks, K = _volume_case(model, htable500, config)
    ae = amico_amd.Evaluation()
    if config == 'raw':
        ae.set_config('doNormalizeSignal', False)
    ae.set_data(img, sch, mask, peaks)
    ae.set_model(model)
    ae.set_kernels(K, ht)
    res = ae.fit()
    sel = mask == 1
    y_ref, _ = signal_np.prepare_signal(img, mask, sch.b0_idx, sch.dwi_idx, do_normalize=(config != 'raw'))
    assert np.array_equal(ae.y, y_ref)
    amp = y_ref.max(axis=1)
    print('AMPLITUDE %s %s: %d voxels, max signal %.3e, voxels above 100: %d' % (model, config, len(y_ref), amp.max(), int((amp > 100).sum())))
    if config == 'tiny b0':
        assert amp.max() > 1e3 and (amp > 100).sum() > 0.01 * len(y_ref)
    d_ref = peaks.astype(np.float32)[sel].astype(np.float64)             # peaks are float32 (core.py:442)
    if model == 'NODDI':
        assert len(y_ref) >= 30_000
        ref = oracle.noddi_fit(y_ref, d_ref, K, ht, sch.dwi_idx, nthreads=NTHREADS)
    else:
        ref = oracle.freewater_fit(y_ref, d_ref, K, ht, nthreads=NTHREADS)
    assert ref['err'] == 0
    diff = np.abs(res['estimates'] - ref['estimates']).max(axis=1)
    print('AMPLITUDE %s %s vs oracle: max %.3e, > 1e-6: %d, worst voxel amplitude %.3e'
          % (model, config, diff.max(), int((diff > 1e-6).sum()), amp[int(diff.argmax())]))
    assert diff.max() <= CAP, (model, config, float(diff.max()), float(amp[int(diff.argmax())]))
