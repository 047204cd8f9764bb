"""k_lasso_seed takes the atoms that leave from the dual scan: the scan, which forms s_j'r of every atom on the matrix cores, also says
for every PASSIVE atom whether t_j = s_j'r - lambda1 <= 0 -- one 64-bit word of verdicts per lane and voxel group, exchanged between the
four rows of a column and unpacked into the layout of P (LeavePack, amx_seed.hpp) -- where a per-lane loop over the set bits of P
computed every t_j again.  Both builds of the kernel (two wavefronts per SIMD; one wavefront with the next voxel reserved) on 24 576
voxels, the smallest call that takes the seeded chain by default (AMX_SEED_MIN_VOXELS = 22 528):

  (a) the benchmark's signal mix and (b) synthetic.noddi_hard_signals: maps within 1e-6 of the oracle on EVERY voxel,
      and the device's LASSO coefficient vectors pass tests/kkt_certificates.py at 1e-9 (a) / 4e-9 (b);
  (c) lambda1 = 0.2: supports beyond the seed solver's 20 atoms, so the give-up path -- a full set with candidates left -- runs: maps
      against the oracle, no overflow;
  (d) a NaN and an Inf sample in two voxels of (a): NaN maps there, every other voxel the same bits as without them;
  (e) the same call twice: the same bits; (f) both builds: the same maps;
  (g) a dictionary of 100 white-matter atoms -- no multiple of 16, so the last scan tile is partly padding, and its second mask word
      ends at bit 35: another split of the verdict word than the default 144 atoms' -- with the checks of (a) and (b), in one build;
  (h) 22 528 + 7 voxels that all have ONE orientation: the chunks of that orientation end in partly filled wavefronts, where the
      scan runs for fewer than four voxel groups (GN < 4) and the rest of the lanes are idle: maps against the oracle on every voxel.
"""
import os

import numpy as np
import pytest

from kkt_certificates import noddi_certificates

pytestmark = pytest.mark.gpu

N_VOX = 24576
N_TAIL = 22528 + 7
TOL = 1e-6                      # the project's bar for the maps
KKT_CLEAN, KKT_HARD = 1e-9, 4e-9
LAMBDA1_WIDE = 0.2
BAD = (777, 20001)              # (d): voxel with a NaN sample, voxel with an Inf sample
BUILDS = {'occ2': '1', 'one wavefront': '1000000000'}        # AMX_SEED2_OCC2_FROM
BUILD_100 = 'occ2'              # (g) runs in this build


@pytest.fixture(scope='module')
def runs():
    """every fit of this file, made once: {'ref': {batch: oracle maps}, 'data': {batch: (K, y, d)}, build: {batch: {'maps', 'x', 'seed', 'stats', 'path'}}}"""
    import torch
    from amico_amd import _capi, synthetic as S
    from oracle import oracle
    dirs = S.fibonacci_hemisphere(500); ht = S.build_htable(dirs); sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, dirs)
    K100 = S.noddi_kernels(sch, dirs, IC_VFs=np.linspace(0.1, 0.99, 10), IC_ODs=np.hstack((np.array([0.03, 0.06]), np.linspace(0.09, 0.99, 8))))
    assert K['wm'].shape[0] == 144 and K100['wm'].shape[0] == 100
    ya, da = S.noddi_signals(N_VOX, K, ht, sch, seed=1)
    yh, dh, _ = S.noddi_hard_signals(N_VOX, K, ht, sch, seed=9)
    yb = ya.copy(); yb[BAD[0], 40] = np.nan; yb[BAD[1], 7] = np.inf
    ya1, da1 = S.noddi_signals(N_VOX, K100, ht, sch, seed=2)
    yh1, dh1, _ = S.noddi_hard_signals(N_VOX, K100, ht, sch, seed=10)
    yt, dt = S.noddi_signals(N_TAIL, K, ht, sch, seed=3)
    dt = np.ascontiguousarray(np.broadcast_to(dt[0], dt.shape))          # one orientation for all voxels
    nt = min(16, os.cpu_count() or 1)
    data = {'mix': (K, ya, da), 'hard': (K, yh, dh), 'mix100': (K100, ya1, da1), 'hard100': (K100, yh1, dh1), 'tail': (K, yt, dt)}
    out = {'ht': ht, 'sch': sch, 'data': data,
           'ref': {name: oracle.noddi_fit(y, d, Kx, ht, sch.dwi_idx, nthreads=nt)['estimates'] for name, (Kx, y, d) in data.items()}}
    out['ref']['wide'] = oracle.noddi_fit(ya, da, K, ht, sch.dwi_idx, nthreads=nt, lambda1=LAMBDA1_WIDE, return_x=True)
    dev = torch.device('cuda', 0)
    mp = pytest.MonkeyPatch()
    try:
        for build, occ in BUILDS.items():
            mp.setenv('AMX_SEED2_OCC2_FROM', occ)
            ctx = _capi.Context(-1)                              # (the switch table is read when a context is created)
            luts = {id(K): _capi.upload_noddi(ctx, K, ht, sch.dwi_idx)}
            if build == BUILD_100:
                luts[id(K100)] = _capi.upload_noddi(ctx, K100, ht, sch.dwi_idx)
            calls = {'mix': (K, ya, da, 0.5), 'again': (K, ya, da, 0.5), 'bad': (K, yb, da, 0.5), 'hard': (K, yh, dh, 0.5),
                     'wide': (K, ya, da, LAMBDA1_WIDE), 'tail': (K, yt, dt, 0.5)}
            if build == BUILD_100:
                calls.update({'mix100': (K100, ya1, da1, 0.5), 'hard100': (K100, yh1, dh1, 0.5)})
            fits = {}
            for name, (Kx, y, d, lam1) in calls.items():
                res = _capi.noddi_fit_device(ctx, luts[id(Kx)], torch.from_numpy(y).to(dev), torch.from_numpy(d).to(dev), lam1, 1e-3, 3, return_x=True)
                ctx.sync()
                fits[name] = {'maps': res[0].cpu().numpy(), 'x': res[-1].cpu().numpy() if name in ('mix', 'hard', 'mix100', 'hard100') else None,
                              'seed': ctx.last_seed_stats(), 'stats': ctx.last_stats(), 'path': ctx.last_path(), 'n': y.shape[0]}
                print('LASSO SEED LEAVE %-14s %-7s leftover_lasso %d of %d  %s' % (build, name, fits[name]['seed']['leftover_lasso'], y.shape[0], fits[name]['seed']))
            out[build] = fits
            for lut in luts.values():
                lut.close()
            ctx.close()
    finally:
        mp.undo()
    return out


def _cases():
    return [(b, n) for b in BUILDS for n in ('mix', 'hard', 'tail') + (('mix100', 'hard100') if b == BUILD_100 else ())]


@pytest.mark.parametrize('build', list(BUILDS))
def test_the_build_ran_in_the_seeded_chain(runs, build):
    for name, fit in runs[build].items():
        assert ('k_lasso_seed<occ2>' in fit['path']) == (build == 'occ2') and 'k_lasso_seed' in fit['path'], (name, fit['path'])
        assert fit['seed']['seeded_voxels'] == fit['n'], (name, fit['seed'])


@pytest.mark.parametrize('build,batch', _cases())
def test_maps_equal_the_oracle_on_every_voxel(runs, build, batch):
    fit = runs[build][batch]
    diff = np.abs(fit['maps'] - runs['ref'][batch]).max(axis=1)          # (no voxel is left out: a NaN here fails the comparison)
    print('LASSO SEED LEAVE %-14s %-7s max |dmap| %.3e  > 1e-6: %d' % (build, batch, diff.max(), int((diff > TOL).sum())))
    assert np.isfinite(fit['maps']).all()
    assert diff.max() < TOL, (float(diff.max()), int(diff.argmax()))
    st = fit['stats']
    assert st['overflow_voxels'] == 0 and st['itercap_voxels'] == 0 and st['guard_trips'] == 0, st


@pytest.mark.parametrize('build,batch', [c for c in _cases() if c[1] != 'tail'])
def test_lasso_coefficients_pass_the_kkt_certificates(runs, build, batch):
    Kx, y, d = runs['data'][batch]
    c = noddi_certificates(Kx, runs['sch'], runs['ht'], y, d, runs[build][batch]['x'], 0.5, 1e-3)
    print('LASSO SEED LEAVE %-14s %-7s %s' % (build, batch, c))
    tol = KKT_CLEAN if batch.startswith('mix') else KKT_HARD
    assert c['min_x'] >= 0.0, c
    assert c['s2_gP'] < tol and c['s2_gZ'] < tol, c


@pytest.mark.parametrize('build', list(BUILDS))
def test_supports_beyond_the_seed_solvers_capacity(runs, build):
    """(c): the oracle's supports exceed 20 atoms in some voxels, so those voxels are given up by the seed solver and solved downstream"""
    ref = runs['ref']['wide']
    n_wm = runs['data']['mix'][0]['wm'].shape[0]
    size = (ref['x'][:, 1, :n_wm] > 0).sum(axis=1)
    assert (size > 20).sum() > N_VOX // 50, int((size > 20).sum())
    fit = runs[build]['wide']
    diff = np.abs(fit['maps'] - ref['estimates']).max(axis=1)
    print('LASSO SEED LEAVE %-14s wide    max |dmap| %.3e, supports beyond 20 atoms: %d, leftover_lasso %d' % (
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
    for name in ('mix', 'hard', 'wide', 'tail'):
        assert np.array_equal(runs['occ2'][name]['maps'], runs['one wavefront'][name]['maps']), name
