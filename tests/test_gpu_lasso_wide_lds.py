"""The second LASSO certificate pass (k_lasso_gcert<18, wide>) reads the white-matter Gram block from LDS.

A workgroup of the pass stages the packed lower triangle of its orientation's 144 x 144 Gram block -- tri(i, j) = i (i + 1) / 2 + j,
83 520 B -- beside its other tables and gathers every G_PP and G_tP entry from there instead of from global memory.  Same values, same
arithmetic, same order: what the pass certifies, refuses and hands on is what the commit before it (ded6bea) certified, refused and handed on.

One call of 6 000 voxels of the benchmark's signal mix on THREE orientations (2 000 voxels each, ~19 % of them with a LASSO support of
12 .. 18 atoms by the oracle), so that workgroups stage three different triangles, plus one voxel of the hard mix whose stage-2 signal
clips (the compact table of the exact pass, Cb2).  The oracle's supports must hold every corner of the packed layout: sizes exactly 12
and 18, atom 0 (first packed row), atom 143 (last), both of atoms 63 / 64 and both of 127 / 128.

Then the list lengths at the edges of a block of 64 lanes: calls in which the first orientation holds exactly 1, 63, 64 and 65 voxels,
all with supports of 12 .. 18 atoms (each of them is in the first pass's left-over list: that pass holds 11 atoms), the second none
of that kind (64 voxels with supports of at most 6 atoms), the third as it was.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_MAPS = 1e-6          # the project's bar for the maps
TOL_X = 1e-7             # ... and for the stage-2 coefficients (tests/test_gpu_solvers.py)
ORI = (3, 250, 496)      # three orientations of the 500 that map to themselves
N, SEED = 6000, 6        # (the oracle decides which seed holds every case below; 6 is the first of 1 .. 8 that does)
HARD_N, HARD_SEED, HARD_VOX = 6000, 9, 4328      # a voxel of synthetic.noddi_hard_signals that clips in stage 2 on a support of 12 atoms at ORI[0]
EDGES = (1, 63, 64, 65)
WIDE_NOTE = 'k_lasso_gcert<18,wide>'
# seed_chain.leftover_lasso of the parent commit (ded6bea: the triangle gathered from global memory) for the same inputs: the
# decisions are bit-identical, so the margin is zero
PARENT_LEFTOVER_LASSO = {'all': 42, 1: 16, 63: 16, 64: 16, 65: 16}


def _wide(size):
    return (size >= 12) & (size <= 18)


@pytest.fixture(scope='module')
def problem():
    from amico_amd import synthetic as S
    from oracle import oracle
    dirs = S.fibonacci_hemisphere(500)
    ht = np.asarray(S.build_htable(dirs))
    sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, dirs)
    n_wm = K['wm'].shape[0]
    assert n_wm == 144 and (S.lut_indices(dirs[list(ORI)], ht) == np.array(ORI)).all()
    # the signal mix with every direction cell mapped to one of the three orientations; the fit gets the orientation's own unit vector
    ht3 = np.asarray(ORI)[ht % 3].astype(ht.dtype)
    y, d = S.noddi_signals(N, K, ht3, sch, seed=SEED)
    ori = S.lut_indices(d, ht3)
    yh = S.noddi_hard_signals(HARD_N, K, ht, sch, seed=HARD_SEED)[0][HARD_VOX]
    y = np.ascontiguousarray(np.vstack([y, yh[None]]))
    ori = np.append(ori, ORI[0])
    d = np.ascontiguousarray(dirs[ori])
    assert (S.lut_indices(d, ht) == ori).all()
    ref = oracle.noddi_fit(y, d, K, ht, sch.dwi_idx, nthreads=8, return_x=True)
    x2 = ref['x'][:, 1, :n_wm]
    iso, dwi = K['iso'].astype(np.float64), np.asarray(sch.dwi_idx)
    clipped = ((y[:, dwi] - ref['x'][:, 0, n_wm][:, None] * iso[None, dwi]) < 0).any(axis=1)       # models.pyx:917-925
    return dict(K=K, ht=ht, sch=sch, y=y, d=d, ori=ori, ref=ref, supp=x2 > 0, size=(x2 > 0).sum(axis=1), clipped=clipped, n_wm=n_wm)


def _edge_input(p, n_first):
    """voxel indices: n_first wide voxels at ORI[0], 64 voxels of at most 6 atoms at ORI[1], ORI[2] whole"""
    wide = _wide(p['size'])
    first = np.flatnonzero(wide & (p['ori'] == ORI[0]) & ~p['clipped'])[:n_first]
    second = np.flatnonzero((p['size'] <= 6) & (p['ori'] == ORI[1]))[:64]
    third = np.flatnonzero(p['ori'] == ORI[2])
    assert len(first) == n_first and len(second) == 64
    take = np.concatenate([first, second, third])
    np.random.default_rng(n_first).shuffle(take)
    return take


@pytest.fixture(scope='module')
def runs(problem):
    """{'all' | 1 | 63 | 64 | 65: {'take', 'maps', 'x2', 'seed', 'stats', 'path'}}: every fit of this file, made once"""
    import torch
    from amico_amd import _capi
    p = problem
    dev = torch.device('cuda', 0)
    out = {}
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv('AMX_SEED_MIN_VOXELS', '1')                    # the seeded chain runs at this size (read when a context is created)
        ctx = _capi.Context(-1)
        lut = _capi.upload_noddi(ctx, p['K'], p['ht'], p['sch'].dwi_idx)
        for key in ('all',) + EDGES:
            take = np.arange(len(p['y'])) if key == 'all' else _edge_input(p, key)
            yt = torch.from_numpy(np.ascontiguousarray(p['y'][take])).to(dev)
            dt = torch.from_numpy(np.ascontiguousarray(p['d'][take])).to(dev)
            est, _, _, _, xd = _capi.noddi_fit_device(ctx, lut, yt, dt, 0.5, 1e-3, 3, return_x=True)
            ctx.sync()
            out[key] = {'take': take, 'maps': est.cpu().numpy(), 'x2': xd.cpu().numpy()[:, 1, :p['n_wm']], 'seed': ctx.last_seed_stats(),
                        'stats': ctx.last_stats(), 'path': ctx.last_path()}
        lut.close()
        ctx.close()
    finally:
        mp.undo()
    return out


def test_the_oracle_supports_hold_every_corner_of_the_packed_triangle(problem):
    p = problem
    wide = _wide(p['size'])
    s = p['supp'][wide]
    print('WIDE LDS: %d of %d voxels with 12 .. 18 atoms; per orientation %s' % (wide.sum(), len(wide), [int((wide & (p['ori'] == o)).sum()) for o in ORI]))
    assert 0.15 < wide.mean() < 0.25                             # about a fifth
    assert all((wide & (p['ori'] == o)).sum() > 300 for o in ORI)
    assert (p['size'] == 12).any() and (p['size'] == 18).any()
    assert s[:, 0].any() and s[:, 143].any()
    assert (s[:, 63] & s[:, 64]).any() and (s[:, 127] & s[:, 128]).any()
    assert wide[-1] and p['clipped'][-1]                         # the hard-mix voxel clips in stage 2 on a support this pass holds


@pytest.mark.parametrize('key', ('all',) + EDGES)
def test_the_wide_pass_ran_and_the_chain_took_every_voxel(runs, key):
    r = runs[key]
    assert WIDE_NOTE in r['path'], r['path']
    assert r['seed']['seeded_voxels'] == len(r['take']), r['seed']
    st = r['stats']
    assert st['itercap_voxels'] == 0 and st['overflow_voxels'] == 0 and st['guard_trips'] == 0, st
    if key == 'all':
        assert r['seed']['clipped_stage2'] >= 1, r['seed']


@pytest.mark.parametrize('key', ('all',) + EDGES)
def test_maps_and_stage2_coefficients_of_the_wide_supports_equal_the_oracle(problem, runs, key):
    p, r = problem, runs[key]
    sel = _wide(p['size'][r['take']])
    assert sel.any()
    dm = np.abs(r['maps'] - p['ref']['estimates'][r['take']]).max(axis=1)
    dx = np.abs(r['x2'] - p['ref']['x'][r['take'], 1, :p['n_wm']]).max(axis=1)
    print('WIDE LDS %-4s %5d wide voxels: max |dmap| %.3e  max |dx2| %.3e   (all %d voxels: %.3e, %.3e)'
          % (key, sel.sum(), dm[sel].max(), dx[sel].max(), len(sel), dm.max(), dx.max()))
    assert dm[sel].max() < TOL_MAPS, (float(dm[sel].max()), int(r['take'][sel][dm[sel].argmax()]))
    assert dx[sel].max() < TOL_X, (float(dx[sel].max()), int(r['take'][sel][dx[sel].argmax()]))


@pytest.mark.parametrize('key', ('all',) + EDGES)
def test_leftover_count_equals_the_parent_commits(runs, key):
    print('WIDE LDS %-4s %s' % (key, runs[key]['seed']))
    assert runs[key]['seed']['leftover_lasso'] == PARENT_LEFTOVER_LASSO[key], (key, runs[key]['seed'])
