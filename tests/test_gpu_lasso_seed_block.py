"""k_lasso_seed's trip -- every passive atom with t_j <= 0 leaves, up to four candidates of the scan's pool enter, M and g take the
changes and ONE factorisation follows -- in both builds of the kernel (two wavefronts per SIMD, and the one-wavefront build with the
next voxel reserved), on 24 576 voxels: the smallest call that takes the seeded chain by default (AMX_SEED_MIN_VOXELS = 22 528).

  (a) the benchmark's signal mix and (b) synthetic.noddi_hard_signals (wide supports, CSF, noise, flat, half-zeroed): maps within
      1e-6 of the oracle on EVERY voxel, and the device's LASSO coefficient vectors pass tests/kkt_certificates.py at
      the bounds of tests/test_gpu_kkt.py (1e-9 on clean data, 4e-9 on the hard mix);
  (c) lambda1 = 0.2: the oracle's LASSO supports exceed the seed solver's 20 atoms in 8 % of these voxels (0.5: 17 voxels; measured on
      the CPU oracle), so the give-up path -- a full set with candidates left -- runs: maps against the oracle, no overflow;
  (d) a NaN and an Inf sample in two voxels of (a): NaN maps there, every other voxel the same bits as without them;
  (e) the same call twice: the same bits;
  (f) ctx.last_seed_stats()['leftover_lasso'] of every fit is printed.
"""
import os

import numpy as np
import pytest

from kkt_certificates import noddi_certificates

pytestmark = pytest.mark.gpu

N_VOX = 24576
TOL = 1e-6                      # the project's bar for the maps
KKT_CLEAN, KKT_HARD = 1e-9, 4e-9
LAMBDA1_WIDE = 0.2
BAD = (777, 20001)              # (d): voxel with a NaN sample, voxel with an Inf sample
BUILDS = {'occ2': '1', 'one wavefront': '1000000000'}        # AMX_SEED2_OCC2_FROM


@pytest.fixture(scope='module')
def runs():
    """every fit of this file, made once: {'ref': {batch: oracle maps}, 'data': .., build: {batch: {'maps', 'x', 'seed', 'stats', 'path'}}}"""
    import torch
    from amico_amd import _capi, synthetic as S
    from oracle import oracle
    dirs = S.fibonacci_hemisphere(500); ht = S.build_htable(dirs); sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, dirs)
    ya, da = S.noddi_signals(N_VOX, K, ht, sch, seed=1)
    yh, dh, _ = S.noddi_hard_signals(N_VOX, K, ht, sch, seed=9)
    yb = ya.copy(); yb[BAD[0], 40] = np.nan; yb[BAD[1], 7] = np.inf
    nt = min(16, os.cpu_count() or 1)
    out = {'K': K, 'ht': ht, 'sch': sch, 'data': {'mix': (ya, da), 'hard': (yh, dh)},
           'ref': {'mix': oracle.noddi_fit(ya, da, K, ht, sch.dwi_idx, nthreads=nt)['estimates'],
                   'hard': oracle.noddi_fit(yh, dh, K, ht, sch.dwi_idx, nthreads=nt)['estimates'],
                   'wide': oracle.noddi_fit(ya, da, K, ht, sch.dwi_idx, nthreads=nt, lambda1=LAMBDA1_WIDE, return_x=True)}}
    dev = torch.device('cuda', 0)
    mp = pytest.MonkeyPatch()
    try:
        for build, occ in BUILDS.items():
            mp.setenv('AMX_SEED2_OCC2_FROM', occ)
            ctx = _capi.Context(-1)                              # (the switch table is read when a context is created)
            lut = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx)
            fits = {}
            for name, (y, d, lam1) in {'mix': (ya, da, 0.5), 'again': (ya, da, 0.5), 'bad': (yb, da, 0.5), 'hard': (yh, dh, 0.5),
                                       'wide': (ya, da, LAMBDA1_WIDE)}.items():
                res = _capi.noddi_fit_device(ctx, lut, torch.from_numpy(y).to(dev), torch.from_numpy(d).to(dev), lam1, 1e-3, 3, return_x=True)
                ctx.sync()
                fits[name] = {'maps': res[0].cpu().numpy(), 'x': res[-1].cpu().numpy() if name in ('mix', 'hard') else None,
                              'seed': ctx.last_seed_stats(), 'stats': ctx.last_stats(), 'path': ctx.last_path()}
                print('LASSO SEED BLOCK %-14s %-6s leftover_lasso %d of %d  %s' % (build, name, fits[name]['seed']['leftover_lasso'], N_VOX, fits[name]['seed']))
            out[build] = fits
            lut.close()
            ctx.close()
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize('build', list(BUILDS))
def test_the_build_ran_in_the_seeded_chain(runs, build):
    for name, fit in runs[build].items():
        assert ('k_lasso_seed<occ2>' in fit['path']) == (build == 'occ2') and 'k_lasso_seed' in fit['path'], (name, fit['path'])
        assert fit['seed']['seeded_voxels'] == N_VOX, (name, fit['seed'])


@pytest.mark.parametrize('batch', ['mix', 'hard'])
@pytest.mark.parametrize('build', list(BUILDS))
def test_maps_equal_the_oracle_on_every_voxel(runs, build, batch):
    fit = runs[build][batch]
    diff = np.abs(fit['maps'] - runs['ref'][batch]).max(axis=1)          # (no voxel is left out: a NaN here fails the comparison)
    print('LASSO SEED BLOCK %-14s %-6s max |dmap| %.3e  > 1e-6: %d' % (build, batch, diff.max(), int((diff > TOL).sum())))
    assert np.isfinite(fit['maps']).all()
    assert diff.max() < TOL, (float(diff.max()), int(diff.argmax()))
    st = fit['stats']
    assert st['overflow_voxels'] == 0 and st['itercap_voxels'] == 0 and st['guard_trips'] == 0, st


@pytest.mark.parametrize('batch', ['mix', 'hard'])
@pytest.mark.parametrize('build', list(BUILDS))
def test_lasso_coefficients_pass_the_kkt_certificates(runs, build, batch):
    y, d = runs['data'][batch]
    c = noddi_certificates(runs['K'], runs['sch'], runs['ht'], y, d, runs[build][batch]['x'], 0.5, 1e-3)
    print('LASSO SEED BLOCK %-14s %-6s %s' % (build, batch, c))
    tol = KKT_CLEAN if batch == 'mix' else KKT_HARD
    assert c['min_x'] >= 0.0, c
    assert c['s2_gP'] < tol and c['s2_gZ'] < tol, c


@pytest.mark.parametrize('build', list(BUILDS))
def test_supports_beyond_the_seed_solvers_capacity(runs, build):
    """(c): the oracle's supports exceed 20 atoms in some voxels, so those voxels are given up by the seed solver and solved downstream"""
    ref = runs['ref']['wide']
    n_wm = runs['K']['wm'].shape[0]
    size = (ref['x'][:, 1, :n_wm] > 0).sum(axis=1)
    assert (size > 20).sum() > N_VOX // 50, int((size > 20).sum())
    fit = runs[build]['wide']
    diff = np.abs(fit['maps'] - ref['estimates']).max(axis=1)
    print('LASSO SEED BLOCK %-14s wide   max |dmap| %.3e, supports beyond 20 atoms: %d, leftover_lasso %d' % (
        build, diff.max(), int((size > 20).sum()), fit['seed']['leftover_lasso']))
    assert diff.max() < TOL, (float(diff.max()), int(diff.argmax()))
    assert fit['stats']['overflow_voxels'] == 0 and fit['stats']['itercap_voxels'] == 0, fit['stats']


@pytest.mark.parametrize('build', list(BUILDS))
def test_nan_and_inf_samples_touch_their_own_voxels_only(runs, build):
    clean, bad = runs[build]['mix']['maps'], runs[build]['bad']['maps']
    assert np.isnan(bad[list(BAD)]).all(), bad[list(BAD)]
    others = np.ones(N_VOX, bool); others[list(BAD)] = False
    assert np.array_equal(bad[others], clean[others])


@pytest.mark.parametrize('build', list(BUILDS))
def test_the_same_call_twice_gives_the_same_bits(runs, build):
    assert np.array_equal(runs[build]['mix']['maps'], runs[build]['again']['maps'])
    assert runs[build]['mix']['seed'] == runs[build]['again']['seed']


def test_both_builds_give_the_same_maps(runs):
    for name in ('mix', 'hard', 'wide'):
        assert np.array_equal(runs['occ2'][name]['maps'], runs['one wavefront'][name]['maps']), name
