"""The trip rule of k_lasso_seed, emulated in numpy (tools/lab/s2_block_lab.py): every passive atom with t_j <= 0 leaves and, in the
same trip, up to four candidates of the scan's pool enter.

On 100 voxels of the benchmark's signal mix every voxel must stop within the kernel's trip cap (20) on exactly the support of the exact
LASSO solution (the oracle's stage-2 coefficients of the full 90-row problem), and the rule must need fewer trips on these voxels than the
rule it replaces (two enter, or one leaves and one enters).  Both pools are held to this: the two best of each row class (the proposal
the rule was designed with) and the best of each (row class, tile parity) group, which is what the kernel keeps.
"""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VOX, RANK, TRIP_CAP = 100, 8, 20


@pytest.fixture(scope='module')
def lab():
    spec = importlib.util.spec_from_file_location('s2_block_lab', os.path.join(ROOT, 'tools', 'lab', 's2_block_lab.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def voxels(lab):
    """[(S2 [8][144], y2~ [8], exact support)] of the 100 voxels: the exact support is the oracle's"""
    from amico_amd import synthetic as S
    from oracle import oracle
    dirs = S.fibonacci_hemisphere(500); ht = S.build_htable(dirs); sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, dirs)
    y, d = S.noddi_signals(N_VOX, K, ht, sch, seed=3)
    x = oracle.noddi_fit(y, d, K, ht, sch.dwi_idx, nthreads=4, return_x=True)['x']
    lut = S.lut_indices(d, ht)
    wm, iso = K['wm'], K['iso'].astype(np.float64)
    n_wm = wm.shape[0]
    dwi = np.asarray(sch.dwi_idx); norms = K['norms'][0]
    out = []
    for v in range(N_VOX):
        A2 = wm[:, lut[v], :].astype(np.float64).T[dwi] * norms[None, :]
        U2 = lab.rrqr(A2, RANK)
        y2 = np.maximum(y[v][dwi] - x[v, 0, n_wm] * iso[dwi], 0.0)          # models.pyx:917-925
        out.append((U2.T @ A2, U2.T @ y2, x[v, 1, :n_wm] > 0))
    return out


@pytest.fixture(scope='module')
def runs(lab, voxels):
    rules = {'kernel': ('kernel',), 'block': ('block', 4, True), 'groups': ('groups', 4, True)}
    # (no limit on the size of the set: a voxel that fills the kernel's 20 slots and wants more is given up there, which the GPU test covers)
    return {name: [lab.trips(S2, yt, rule, cap=10 * TRIP_CAP) for S2, yt, _ in voxels] for name, rule in rules.items()}


@pytest.mark.parametrize('rule', ['block', 'groups'])
def test_every_voxel_stops_within_the_trip_cap(runs, rule):
    nt = np.array([r[1] for r in runs[rule]])
    print('LASSO SEED RULE %-6s trips mean %.2f p95 %.0f max %d' % (rule, nt.mean(), np.percentile(nt, 95), nt.max()))
    assert nt.max() <= TRIP_CAP, (rule, int(nt.argmax()), int(nt.max()))


@pytest.mark.parametrize('rule', ['block', 'groups'])
def test_every_voxel_ends_on_the_exact_support(runs, voxels, rule):
    wrong = [v for v, (r, (_, _, P2)) in enumerate(zip(runs[rule], voxels)) if not (r[0] == P2).all()]
    assert not wrong, (rule, wrong)


@pytest.mark.parametrize('rule', ['block', 'groups'])
def test_fewer_trips_than_the_rule_it_replaces(runs, rule):
    new = np.mean([r[1] for r in runs[rule]]); old = np.mean([r[1] for r in runs['kernel']])
    print('LASSO SEED RULE %-6s mean trips %.2f, replaced rule %.2f' % (rule, new, old))
    assert new < old, (rule, new, old)
