"""The yardstick of test_gpu_noddi_hard.py, pinned on the CPU: on the hard voxels of noddi_np.hard_signals -- crossings, the wrong
direction, pure noise, flat, half zeroed, CSF dominated, background, all-zero, amplitudes 2^-8 / 1 / 2^6 side by side -- and on every
dictionary, protocol and lambda pair of noddi_np.CASES

* the CPU oracle's own coefficients meet the per-voxel certificate the device is held to (kkt_certificates.noddi_certificates_per_voxel:
  long-double residuals, relative to s = max|y| of the voxel) with two digits to spare: every value < 1e-11 s (measured: <= 1.3e-12, v512);
* noddi_np.noddi_maps of its stage-3 coefficients are its maps to 1e-12 relative, rmse_ld / nrmse_ld its error maps;
* at most 1 % of the voxels are degenerate for the oracle (a stage-2 coefficient or a clamped atom's dual value within 1e-7 s of zero;
  measured: 1 .. 19 of 3 000 at lambda2 = 1e-3, 12 .. 23 at lambda2 = 1e-6);
* the route of every case without a switch of its own is what the table expects (_capi.noddi_route, no device);
* the mix does what it is there for: a voxel with an empty LASSO support, one with more than 18 atoms, one with more than 64
  (measured: up to 139 atoms; the cases of noddi_np.NO_DENSE cannot have them).

A second test shows that the certificate has teeth."""
import numpy as np
import pytest

import noddi_np as N


@pytest.mark.parametrize('name', list(N.CASES))
def test_case_table(name):
    c = N.CASES[name]
    sch, K = N.dictionary(name)
    n_wm = K['wm'].shape[0]
    assert n_wm == c['grid'][0] * c['grid'][1] and list(sch.b0_idx) == list(range(sch.b0_count))
    if c['route'] is not None:
        assert not c['env']
        rt = N.route_of(name)
        assert {k: rt[k] for k in c['route']} == c['route'], (name, {k: rt[k] for k in c['route']})
        assert rt['seeds'] == c['seeded']
        # (a call of 100 000 voxels launches the occ2 seed builds, one of 3 000 does not: the names before the first comma or bracket)
        path = rt['path'] + ' ->'
        assert all(m in path for m in c['must']) and not any(m in path for m in c['must_not']), (name, rt['path'])
    else:
        assert c['env'] and c['must']
    assert c['n'] in (N.N_SMALL, N.BIG_N) and (c['n'] == N.N_SMALL or (not c['env'] and c['signals'] in N.CASES))


def test_the_lds_edge_is_the_routes_own():
    from amico_amd import _capi
    e = N.lds_edge()
    assert 129 <= e < 256
    for nS, want in ((e, False), (e + 1, True)):
        assert _capi.noddi_route(nS, 144, nS - 9, 500, 0, 100_000)['global'] == want
    assert N.dictionary('vLDS')[0].nS == e and N.dictionary('vGT')[0].nS == e + 1
    b0 = {N.dictionary(k)[0].b0_count for k in N.CASES}
    assert 1 in b0 and 18 in b0


@pytest.mark.parametrize('name', N.SMALL_CASES + ['big105'])
def test_oracle_meets_the_standard_on_hard_voxels(name):
    c = N.CASES[name]
    sch, K, y, d, kind, amp = N.problem(name)
    ref = N.reference(name)
    x = ref['x']
    n, n_wm = len(y), K['wm'].shape[0]
    s = N.scale_of(y)
    assert n == N.N_SMALL and not y[:10].any() and (s[10:] > 0).all() and set(kind) == set(range(8)) and sch.nS == y.shape[1]
    from amico_amd import synthetic as S
    lut = S.lut_indices(d, N._htable()['htable'])
    assert [int((lut == o).sum()) for o in N.ORI] == list(N.COUNTS)
    assert len(np.unique(lut[:300])) == 3 and np.array_equal(y, y.astype(np.float32))
    # the certificate of the oracle's own coefficients
    cert = N.reference_certificates(name)
    worst = max(float(cert[k].max()) for k in ('gP1', 'gZ1', 'gP2', 'gZ2', 'gP3', 'gZ3'))
    print('NODDIHARD-CPU %-14s %3d x %3d  oracle gP|gZ / s <= %.1e' % (name, sch.nS, x.shape[2], worst))
    assert not N.kkt_failures(cert, N.ORACLE_KKT).any(), (name, worst)
    assert not x[:10].any()
    # maps and error maps restated from its x
    mine = N.noddi_maps(x[:, 2], K, c['exvivo'])
    assert (np.abs(mine - ref['estimates']) <= 1e-12 * np.abs(mine)).all()
    assert np.array_equal(mine[:10, :3], np.tile([0.0, 1.0, 0.0], (10, 1)))
    g = N.groups_of(K, d, c['exvivo'])
    rms = np.sqrt((y * y).mean(axis=1))
    assert (np.abs(N.rmse_ld(g, y, x[:, 2]) - ref['rmse']) <= 1e-12 * rms).all()
    assert (np.abs(N.nrmse_ld(g, y, x[:, 2]) - ref['nrmse']) <= 1e-12).all()
    # degenerate voxels
    deg = N.degenerate(x[:, 1, :n_wm], cert['g2'], N.DEGENERATE * s).any(axis=1) & (s > 0)
    assert deg.mean() <= N.MAX_SHARE, (name, int(deg.sum()))
    # what the mix is there for
    size = (x[:, 1, :n_wm] > 0).sum(axis=1)
    if c['lam'][0] > 0.0:
        assert (size[s > 0] == 0).any(), name
    if name not in N.NO_DENSE:
        assert (size > 18).any() and (size > 64).any(), (name, int(size.max()))


@pytest.mark.parametrize('name', ['d145', 'd145x', 'v161'])
def test_the_certificate_has_teeth(name):
    """the oracle's coefficients with the largest atom of one stage zeroed, with one clamped atom of a stage set to 1e-7 s, scaled by
    1 + 1e-6, or with a stage-3 atom off the allowed set fail the GPU test's bound on that voxel -- at every amplitude"""
    sch, K, y, d, kind, amp = N.problem(name)
    x = N.reference(name)['x']
    s = N.scale_of(y)
    n_wm = K['wm'].shape[0]
    rows = np.arange(len(y))
    assert not N.kkt_failures(N.certificates(name, x), N.KKT).any()
    for stage in range(3):
        cols = n_wm if stage == 1 else x.shape[2]
        xs = x[:, stage, :cols]
        has = (xs > 0).any(axis=1)
        assert has.sum() > (500 if stage == 1 else 2500)
        bad = x.copy()
        bad[rows, stage, xs.argmax(axis=1)] = 0.0
        assert N.kkt_failures(N.certificates(name, bad), N.KKT)[has].all(), stage
        bad = x.copy()
        bad[:, stage] *= 1.0 + 1e-6
        assert N.kkt_failures(N.certificates(name, bad), N.KKT)[has].all(), stage
        bad = x.copy()
        first = (xs == 0).argmax(axis=1)
        bad[rows, stage, first] = np.where(xs[rows, first] == 0, 1e-7 * s, xs[rows, first])
        assert N.kkt_failures(N.certificates(name, bad), N.KKT)[s > 0].all(), stage
    off = (x[:, 1, :n_wm] == 0) & (x[:, 2, :n_wm] == 0)
    bad = x.copy()
    bad[rows, 2, off.argmax(axis=1)] = 1e-300
    assert (N.certificates(name, bad)['off3'] > 0).all() and N.kkt_failures(N.certificates(name, bad), N.KKT).all()
