"""k_lasso_seed's scan with leaner element work: the leave verdicts are taken for EVERY atom with a constant bit and masked with the
passive bits once per voxel group (LeavePack::pack, amx_seed.hpp) instead of once per element, and a passive atom stays out of the
maxima by its sign bit instead of a select of the high word.  Neither changes which atoms leave or enter, nor any sum or its order: the
fits of tests/test_gpu_lasso_seed_leave.py (its fixture, made once more for this file; both builds of the kernel, 24 576 voxels, the
smallest call that takes the seeded chain by default) must come out as before, and trips with many changes at once -- the change loops
are as they were, and are held to that here -- as the oracle has them:

  (a) the benchmark's signal mix and (b) synthetic.noddi_hard_signals: maps within 1e-6 of the oracle on every voxel, and
      leftover_lasso -- the voxels the LASSO certificates leave to the wavefront-per-voxel kernel -- EQUAL to the counts recorded
      before the change, 138 and 84 (profiles/lasso_seed_leave_ab.txt 6): a sum in another order would move a voxel or two;
  (c) the 22 528 + 7 voxels of one orientation (chunk tail, scans of 1 - 3 voxel groups): the same bound;
  (d) a voxel with a NaN sample: NaN maps there, every other voxel the same bits, and the kernel ends;
  (e) trips with MANY simultaneous changes: signals that are a sum of seven atoms far apart on the grid at SNR 10, lambda1 = 0.3
      (the default is 0.5).  The supports reach the seed solver's 20 atoms, and the trip rule emulated on the CPU (the rule
      'groups', 4 of tools/lab/s2_block_lab.py on 300 of these voxels, seed 5) has trips with four enterers and trips with three or
      more leavers side by side -- see many_atom_signals.  The device's LASSO coefficients pass tests/kkt_certificates.py at the
      level of (b), the maps equal the oracle's.
"""
import os

import numpy as np
import pytest

from kkt_certificates import noddi_certificates
from test_gpu_lasso_seed_leave import BAD, BUILDS, KKT_HARD, N_VOX, TOL, runs      # noqa: F401  (runs: the module's fixture, reused)

pytestmark = pytest.mark.gpu

LEFTOVER_LASSO = {'mix': 138, 'hard': 84}       # the parent's counts (profiles/lasso_seed_leave_ab.txt 6)
LAMBDA1_MANY, SEED_MANY, ATOMS_MANY, SNR_MANY = 0.3, 5, 7, 10.0
MAX_ATOMS = 20                                  # the seed solver's capacity (amx_seed.hip: max_atoms)


def many_atom_signals(n_vox, K, ht, sch, seed=SEED_MANY, n_atoms=ATOMS_MANY, snr=SNR_MANY):
    """(y, DIRs): every voxel a random convex mix of n_atoms white-matter atoms, one from each of n_atoms equal stretches of the atom
    grid (far apart: other orientation dispersions), Rician noise at `snr`.  With lambda1 = 0.3 the sets grow by four atoms a trip
    and shed two or three of them in the next, so a wavefront's lanes hold every mix of leavers and enterers in one trip: of the
    2 458 emulated trips of 300 such voxels (seed 5; 8.4 trips a voxel) 70 % have four enterers and 20 % three or more leavers (up
    to 7), and 7 % of the voxels end with the seed solver's 20 atoms; the oracle's supports hold 20 atoms or more in 8 % of them."""
    from amico_amd import synthetic as S
    rng = np.random.default_rng(seed)
    wm = K['wm']
    dirs = S.random_unit_vectors(n_vox, rng)
    lut = S.lut_indices(dirs, ht)
    width = wm.shape[0] // n_atoms
    k = (np.arange(n_atoms) * width)[None, :] + rng.integers(0, width, (n_vox, n_atoms))
    w = rng.dirichlet(np.ones(n_atoms), n_vox)
    y0 = np.einsum('va,vas->vs', w, wm[k, lut[:, None], :].astype(np.float64))
    return S._finish(S._rician(y0, snr, rng), sch), dirs


@pytest.fixture(scope='module')
def many(runs):
    """case (e): {'y', 'd', 'K', 'ref': oracle (estimates, x), build: {'maps', 'x', 'seed', 'stats', 'path'}}"""
    import torch
    from amico_amd import _capi
    from oracle import oracle
    K = runs['data']['mix'][0]
    ht, sch = runs['ht'], runs['sch']
    y, d = many_atom_signals(N_VOX, K, ht, sch)
    out = {'y': y, 'd': d, 'K': K,
           'ref': oracle.noddi_fit(y, d, K, ht, sch.dwi_idx, nthreads=min(16, os.cpu_count() or 1), lambda1=LAMBDA1_MANY, return_x=True)}
    dev = torch.device('cuda', 0)
    mp = pytest.MonkeyPatch()
    try:
        for build, occ in BUILDS.items():
            mp.setenv('AMX_SEED2_OCC2_FROM', occ)
            ctx = _capi.Context(-1)
            lut = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx)
            res = _capi.noddi_fit_device(ctx, lut, torch.from_numpy(y).to(dev), torch.from_numpy(d).to(dev), LAMBDA1_MANY, 1e-3, 3, return_x=True)
            ctx.sync()
            out[build] = {'maps': res[0].cpu().numpy(), 'x': res[-1].cpu().numpy(), 'seed': ctx.last_seed_stats(), 'stats': ctx.last_stats(),
                          'path': ctx.last_path()}
            print('LASSO SEED TRIP %-14s many    %s' % (build, out[build]['seed']))
            lut.close()
            ctx.close()
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize('build', list(BUILDS))
@pytest.mark.parametrize('batch', ['mix', 'hard'])
def test_the_certificates_leave_the_same_number_of_voxels_as_before(runs, build, batch):
    fit = runs[build][batch]
    print('LASSO SEED TRIP %-14s %-7s leftover_lasso %d (before: %d)' % (build, batch, fit['seed']['leftover_lasso'], LEFTOVER_LASSO[batch]))
    assert ('k_lasso_seed<occ2>' in fit['path']) == (build == 'occ2') and 'k_lasso_seed' in fit['path'], fit['path']
    assert fit['seed']['seeded_voxels'] == N_VOX, fit['seed']
    assert fit['seed']['leftover_lasso'] == LEFTOVER_LASSO[batch], fit['seed']


@pytest.mark.parametrize('build', list(BUILDS))
@pytest.mark.parametrize('batch', ['mix', 'hard', 'tail'])
def test_maps_equal_the_oracle_on_every_voxel(runs, build, batch):
    fit = runs[build][batch]
    diff = np.abs(fit['maps'] - runs['ref'][batch]).max(axis=1)
    print('LASSO SEED TRIP %-14s %-7s max |dmap| %.3e  > 1e-6: %d' % (build, batch, diff.max(), int((diff > TOL).sum())))
    assert 'k_lasso_seed' in fit['path'] and fit['seed']['seeded_voxels'] == fit['n'], (fit['path'], fit['seed'])
    assert np.isfinite(fit['maps']).all()
    assert diff.max() < TOL, (float(diff.max()), int(diff.argmax()))
    st = fit['stats']
    assert st['overflow_voxels'] == 0 and st['itercap_voxels'] == 0 and st['guard_trips'] == 0, st


@pytest.mark.parametrize('build', list(BUILDS))
def test_a_nan_sample_ends_in_its_own_voxel(runs, build):
    """(d): the fit returned, so no lane waited for that voxel; it has NaN maps and no other voxel has other bits"""
    clean, bad = runs[build]['mix'], runs[build]['bad']
    assert np.isnan(bad['maps'][BAD[0]]).all(), bad['maps'][BAD[0]]
    others = np.ones(N_VOX, bool); others[list(BAD)] = False
    assert np.array_equal(bad['maps'][others], clean['maps'][others])
    assert bad['stats']['guard_trips'] == 0 and bad['stats']['itercap_voxels'] == 0, bad['stats']
    # the two bad voxels are either given up by the seed solver (left over) or never reach it: nothing else moves
    extra = bad['seed']['leftover_lasso'] - clean['seed']['leftover_lasso']
    assert 0 <= extra <= len(BAD), (bad['seed'], clean['seed'])


def test_many_changes_supports_reach_the_seed_solvers_capacity(many):
    """(e), on the CPU: the oracle's supports say that the seed solver's sets fill up (and that many atoms come and go on the way)"""
    n_wm = many['K']['wm'].shape[0]
    size = (many['ref']['x'][:, 1, :n_wm] > 0).sum(axis=1)
    print('LASSO SEED TRIP many: oracle support sizes mean %.1f, max %d, >= %d atoms: %d of %d' % (
        size.mean(), size.max(), MAX_ATOMS, int((size >= MAX_ATOMS).sum()), N_VOX))
    assert (size >= MAX_ATOMS).sum() > N_VOX // 50, int((size >= MAX_ATOMS).sum())
    assert np.median(size) >= 8, float(np.median(size))


@pytest.mark.parametrize('build', list(BUILDS))
def test_many_changes_in_one_trip(many, build):
    fit = many[build]
    assert ('k_lasso_seed<occ2>' in fit['path']) == (build == 'occ2') and 'k_lasso_seed' in fit['path'], fit['path']
    assert fit['seed']['seeded_voxels'] == N_VOX, fit['seed']
    diff = np.abs(fit['maps'] - many['ref']['estimates']).max(axis=1)
    assert np.isfinite(fit['maps']).all()
    print('LASSO SEED TRIP %-14s many    max |dmap| %.3e, leftover_lasso %d' % (build, diff.max(), fit['seed']['leftover_lasso']))
    assert diff.max() < TOL, (float(diff.max()), int(diff.argmax()))
    assert fit['stats']['overflow_voxels'] == 0 and fit['stats']['itercap_voxels'] == 0 and fit['stats']['guard_trips'] == 0, fit['stats']


@pytest.mark.parametrize('build', list(BUILDS))
def test_many_changes_lasso_coefficients_pass_the_kkt_certificates(runs, many, build):
    c = noddi_certificates(many['K'], runs['sch'], runs['ht'], many['y'], many['d'], many[build]['x'], LAMBDA1_MANY, 1e-3)
    print('LASSO SEED TRIP %-14s many    %s' % (build, c))
    assert c['min_x'] >= 0.0, c
    assert c['s2_gP'] < KKT_HARD and c['s2_gZ'] < KKT_HARD, c


def test_many_changes_both_builds_give_the_same_maps(many):
    assert np.array_equal(many['occ2']['maps'], many['one wavefront']['maps'])
