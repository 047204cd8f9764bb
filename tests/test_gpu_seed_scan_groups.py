"""The seed solvers' dual scans run for the voxel groups that hold a lane in need of one, not for all 64 columns of the wavefront.

k_nnls_seed<1, 8> and k_lasso_seed compact the lanes that need a scan into the first columns of the scan's B operand, run the
products and the tag / max work for ceil(lanes / 16) voxel groups and hand every result back to the lane that owns the voxel.  A
voxel's dual values depend on its own column alone, so nothing a voxel gets may depend on which lanes work beside it:

  * batch (a): twelve orientations that hold 1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65 and 130 voxels -- the populations on either
    side of every group boundary (a chunk is the voxels of one orientation: those numbers are the lanes at work in its wavefronts);
  * batch (b): 3 000 voxels of the hard signal mix (flat, all-zero, noise, half-zeroed ... voxels) plus NaN / Inf samples, random
    directions;
  * both builds of each kernel (one / two wavefronts per SIMD), one and four wavefronts per workgroup (which voxels share a
    wavefront changes), and every arrangement once more with the voxels in a random order.

The maps must equal the oracle's, and be the same bits in every arrangement; the left-over and clipped counts of the chain must be
the same in every arrangement and equal to what the parent commit counted for these batches -- a scan result that reaches the wrong
lane still ends in right maps (the certificates refuse the seed and the left-over kernels solve the voxel), but not in these counts.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-6            # the project's bar for the maps
POPULATIONS = (1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 130)
N_HARD = 3000
BAD_HARD = (11, 12, N_HARD - 1)          # voxels of batch (b) that get a NaN / +Inf / -Inf sample
# (AMX_SEED_OCC2_FROM = AMX_SEED2_OCC2_FROM, AMX_SEED_WAVES)
ARRANGEMENTS = [('1', '1'), ('1', '4'), ('1000000000', '1'), ('1000000000', '4')]
COUNT_KEYS = ('seeded_voxels', 'leftover_stage1', 'leftover_lasso', 'leftover_stage3', 'clipped_stage2')
# what the parent of the compacted scan (commit 281f8c6) counted for these batches, in every arrangement
PARENT_COUNTS = {
    'groups': {'seeded_voxels': 533, 'leftover_stage1': 30, 'leftover_lasso': 8, 'leftover_stage3': 11, 'clipped_stage2': 1},
    'hard': {'seeded_voxels': 3000, 'leftover_stage1': 53, 'leftover_lasso': 10, 'leftover_stage3': 34, 'clipped_stage2': 471},
}


def _group_batch(K, ht, dirs, sch):
    """batch (a): voxels of noddi_signals whose direction is replaced by the LUT orientation it maps to -- twelve orientations,
    POPULATIONS voxels each, shuffled"""
    from amico_amd import synthetic as S
    y, d = S.noddi_signals(100_000, K, ht, sch, seed=5)
    lut = S.lut_indices(d, ht)
    own = S.lut_indices(dirs, ht) == np.arange(len(dirs))        # orientations that map to themselves
    pop = np.bincount(lut, minlength=len(dirs))
    order = [o for o in np.argsort(-pop, kind='stable') if own[o]]
    take = []
    for o, n in zip(order, sorted(POPULATIONS, reverse=True)):
        members = np.flatnonzero(lut == o)
        assert len(members) >= n, (o, len(members), n)
        take.append(members[:n])
    take = np.concatenate(take)
    np.random.default_rng(2).shuffle(take)
    yb, db = np.ascontiguousarray(y[take]), np.ascontiguousarray(dirs[lut[take]])
    got = np.bincount(S.lut_indices(db, ht), minlength=len(dirs))
    assert sorted(got[got > 0]) == sorted(POPULATIONS) and len(yb) == sum(POPULATIONS)
    return yb, db


@pytest.fixture(scope='module')
def runs():
    """every fit of this file, made once: {batch: {'ref': oracle maps, 'bad': mask, 'fits': {(occ2_from, waves, permuted): ...}}}"""
    from amico_amd import _capi, synthetic as S
    from oracle import oracle
    dirs = S.fibonacci_hemisphere(500)                           # the benchmark's dictionary: 500 orientations, 99 volumes, 145 atoms
    ht = S.build_htable(dirs)
    sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, dirs)
    assert K['wm'].shape[0] + 1 == 145 and len(dirs) == 500
    batches = {}
    yg, dg = _group_batch(K, ht, dirs, sch)
    batches['groups'] = (yg, dg, np.zeros(len(yg), bool))
    yh, dh, _ = S.noddi_hard_signals(N_HARD, K, ht, sch, seed=9)
    yh[BAD_HARD[0]] = np.nan; yh[BAD_HARD[1], 3] = np.inf; yh[BAD_HARD[2], 50] = -np.inf
    bad = np.zeros(N_HARD, bool); bad[list(BAD_HARD)] = True
    batches['hard'] = (yh, dh, bad)
    out = {}
    for name, (y, d, bad) in batches.items():
        ref = oracle.noddi_fit(np.where(bad[:, None], 0.0, y), d, K, ht, sch.dwi_idx, nthreads=8)['estimates']
        out[name] = {'ref': ref, 'bad': bad, 'fits': {}}
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv('AMX_SEED_MIN_VOXELS', '1')                    # the seeded chain runs at this size
        for occ, waves in ARRANGEMENTS:
            mp.setenv('AMX_SEED_OCC2_FROM', occ); mp.setenv('AMX_SEED2_OCC2_FROM', occ); mp.setenv('AMX_SEED_WAVES', waves)
            ctx = _capi.Context(-1)                              # (the switch table is read when a context is created)
            lut = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx)
            for name, (y, d, bad) in batches.items():
                perm = np.random.default_rng(7).permutation(len(y))
                for permuted in (False, True):
                    yy, dd = (np.ascontiguousarray(y[perm]), np.ascontiguousarray(d[perm])) if permuted else (y, d)
                    est = _capi.noddi_fit(ctx, lut, yy, dd, 0.5, 1e-3, 3)[0]
                    if permuted:
                        back = np.empty_like(est); back[perm] = est; est = back
                    out[name]['fits'][(occ, waves, permuted)] = {
                        'maps': est, 'stats': ctx.last_stats(), 'seed': ctx.last_seed_stats(), 'path': ctx.last_path()}
            lut.close()
            ctx.close()
    finally:
        mp.undo()
    return out


def _counts(fit):
    return {k: fit['seed'][k] for k in COUNT_KEYS}


@pytest.mark.parametrize('batch', ['groups', 'hard'])
def test_both_builds_of_both_seed_solvers_ran(runs, batch):
    for (occ, waves, permuted), fit in runs[batch]['fits'].items():
        two = occ == '1'
        assert ('k_nnls_seed<1,8,occ2>' in fit['path']) == two and ('k_nnls_seed<1,8>' in fit['path']) != two, fit['path']
        assert ('k_lasso_seed<occ2>' in fit['path']) == two, fit['path']
        assert 'k_lasso_seed' in fit['path'] and 'k_nnls_seed<3,6>' in fit['path'], fit['path']
        assert fit['seed']['seeded_voxels'] == len(runs[batch]['ref']), fit['seed']


@pytest.mark.parametrize('batch', ['groups', 'hard'])
def test_maps_equal_the_oracle(runs, batch):
    """1e-6 absolute on every finite voxel; a voxel with a non-finite sample gets NaN maps (tests/test_gpu_parity.py)"""
    r = runs[batch]
    ok = ~r['bad']
    for key, fit in r['fits'].items():
        diff = np.abs(fit['maps'][ok] - r['ref'][ok]).max(axis=1)
        print('SCAN GROUPS %-6s %-28s max |dmap| %.3e  > 1e-6: %d' % (batch, key, diff.max(), int((diff > TOL).sum())))
    for key, fit in r['fits'].items():
        assert np.isnan(fit['maps'][r['bad']]).all(), key
        assert np.isfinite(fit['maps'][ok]).all(), key
        diff = np.abs(fit['maps'][ok] - r['ref'][ok]).max(axis=1)
        assert diff.max() < TOL, (key, float(diff.max()), int(diff.argmax()))


@pytest.mark.parametrize('batch', ['groups', 'hard'])
def test_maps_are_the_same_bits_in_every_arrangement(runs, batch):
    fits = runs[batch]['fits']
    first = fits[(ARRANGEMENTS[0][0], ARRANGEMENTS[0][1], False)]['maps']
    for key, fit in fits.items():
        same = np.all((fit['maps'] == first) | (np.isnan(fit['maps']) & np.isnan(first)), axis=1)
        assert same.all(), (key, int((~same).sum()), int(np.flatnonzero(~same)[0]))


@pytest.mark.parametrize('batch', ['groups', 'hard'])
def test_leftover_and_clipped_counts_do_not_depend_on_the_arrangement(runs, batch):
    fits = runs[batch]['fits']
    for key, fit in fits.items():
        print('SCAN GROUPS %-6s %-28s %s' % (batch, key, _counts(fit)))
    first = _counts(fits[(ARRANGEMENTS[0][0], ARRANGEMENTS[0][1], False)])
    for key, fit in fits.items():
        assert _counts(fit) == first, (key, _counts(fit), first)


@pytest.mark.parametrize('batch', ['groups', 'hard'])
def test_counts_equal_the_parent_commits(runs, batch):
    for key, fit in runs[batch]['fits'].items():
        assert _counts(fit) == PARENT_COUNTS[batch], (key, _counts(fit))


@pytest.mark.parametrize('batch', ['groups', 'hard'])
def test_no_voxel_rerun_overflowing_or_guarded(runs, batch):
    for key, fit in runs[batch]['fits'].items():
        st = fit['stats']
        assert st['rerun_voxels'] == 0 and st['overflow_voxels'] == 0 and st['guard_trips'] == 0, (key, st)
