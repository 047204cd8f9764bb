"""The yardstick of test_gpu_small_hard.py, pinned on the CPU: on the hard voxel mix of small_np.hard_mix -- all-zero, exactly one atom,
pure noise, negated, signed, constant, uniform mixture, amplitudes 2^-20 / 1 / 2^20 side by side -- and on every dictionary and
lambda pair of the GPU route table, the CPU oracle itself meets the standard the device routes are held to, with room to spare:

* its Kuhn-Tucker residuals (long-double residual) are at most 1e-12 max|y| on every voxel (the GPU bound is 1e-9 max|y|);
* its supports equal those of czb_np.czb_resolve (block pivoting refined against long-double residuals) on every atom the re-solve
  does not call degenerate, and its x lies within czb_np.x_bound of the re-solve's;
* small_np.fw_maps / sandi_maps of its x are its maps to 1e-13;
* every map of oracle and re-solve agrees to 1e-8 (SANDI's sizes relative, small_np.map_distance).

With lambda2 = 0 no re-solve exists (A'A is singular or at cond 4e16) and x need not be unique: the reference is the oracle's NNLS
(small_np.fw_reference) and is held to its certificate and its maps alone.  A second test shows that the certificate has teeth."""
import numpy as np
import pytest

import czb_np as Z
import small_np as N

N_VOX = 240
PAIRS = [('fw', name, lam) for name, c in N.FW_CASES.items() for lam in c['lams']] + \
        [('sandi', name, lam) for name, c in N.SANDI_CASES.items() for lam in c['lams']]


def _problem(model, name):
    """(groups [(rows, A)], y, kind, reference(lam) -> (x, maps), maps_of(x), n_atoms)"""
    if model == 'fw':
        c = N.FW_CASES[name]
        _, K = N.fw_case_dictionary(c)
        y, d, lut, kind = N.fw_problem(K, counts=(120, 80, 40), seed=1, f32=c['f32'])
        return (N.fw_groups(K, lut), y, kind, lambda lam: N.fw_reference(K, c, lam, y, d, lut),
                lambda x: N.fw_maps(x, c['n_perp'], c['mouse']), K['D'].shape[0] + K['CSF'].shape[0])
    c = N.SANDI_CASES[name]
    _, K, Rs, d_in, d_isos = N.sandi_case_dictionary(c)
    y, kind = N.sandi_problem(K, N_VOX, seed=1, f32=c['f32'], exact=c['exact'])
    return ([(np.arange(N_VOX), N.sandi_matrix(K))], y, kind, lambda lam: N.sandi_reference(K, Rs, d_in, d_isos, lam, y),
            lambda x: N.sandi_maps(x * K['norms'][None, :], len(Rs), len(d_in), Rs, d_in, d_isos), len(K['norms']))


def _resolve(A, y, lam1, lam2, xo):
    """czb_resolve from its own start.  At lambda2 = 5e-10 block pivoting from the signs of c runs out of trips on about one ordinary
    voxel in 240 (the backup rule's single exchanges are finite but not short); such a voxel is re-solved from the oracle's support,
    which the re-solve then confirms or corrects by its own long-double conditions"""
    try:
        return Z.czb_resolve(A, y, lam1, lam2)
    except RuntimeError:
        assert lam2 < 1e-9
        return Z.czb_resolve(A, y, lam1, lam2, start=xo > 0)


@pytest.mark.parametrize('model,name,lam', PAIRS, ids=['%s-%s-%g-%g' % (m, n, l[0], l[1]) for m, n, l in PAIRS])
def test_oracle_meets_the_standard_on_hard_voxels(model, name, lam):
    groups, y, kind, reference, maps_of, n_atoms = _problem(model, name)
    lam1, lam2 = lam
    xo, mo = reference(lam)
    s = N.scale_of(y)
    assert len(y) == N_VOX and set(kind) == set(range(11)) and (s == 0).any() and (s > 1e5).any() and (s < 1e-5).any()
    assert (np.abs(maps_of(xo) - mo) <= 1e-13 * np.maximum(np.abs(mo), 1.0)).all()
    worst = 0.0
    for rows, A in groups:
        gp, gz, mn = N.certificate(A, y[rows], xo[rows], lam1, lam2)
        assert (mn >= 0).all() and (gp <= 1e-12 * s[rows]).all() and (gz <= 1e-12 * s[rows]).all(), (name, lam)
        assert not xo[rows][s[rows] == 0].any()
        if lam2 == 0.0:
            continue
        go = N.gradient(A, y[rows], xo[rows], lam1, lam2)
        for i, v in enumerate(rows):
            xr, gr = _resolve(A, y[v], lam1, lam2, xo[v])
            bound = Z.x_bound(n_atoms, lam2, s[v])
            assert np.abs(xr - xo[v]).max() <= bound, (name, lam, int(v), N.KINDS[kind[v]])
            diff = (xr > 0) != (xo[v] > 0)
            if diff.any():
                deg = N.degenerate(xr[None], gr[None], np.array([bound]))[0]
                assert deg[diff].all(), (name, lam, int(v), N.KINDS[kind[v]], xr[diff], gr[diff], go[i][diff])
            dm = float(N.map_distance(maps_of(xr[None]), mo[v:v + 1])[0])
            worst = max(worst, dm)
            assert dm <= 1e-8, (name, lam, int(v), N.KINDS[kind[v]], dm)
    print('%s %s %s: maps of oracle and re-solve within %.1e' % (model, name, lam, worst))


@pytest.mark.parametrize('model,name', [('fw', 'fused11'), ('fw', 'fused12_f32'), ('fw', 'fused11_lam1'), ('sandi', 'rows'), ('sandi', 'lane15_edge')])
def test_the_certificate_has_teeth(model, name):
    """the oracle's x with one support atom zeroed, with one clamped atom set to 1e-7 max|y|, or scaled by 1 + 1e-6 fails the GPU
    test's bound (small_np.kkt_ok) on that voxel -- every voxel that has a support (and a clamped atom), at every amplitude"""
    groups, y, kind, reference, _, n_atoms = _problem(model, name)
    c = (N.FW_CASES if model == 'fw' else N.SANDI_CASES)[name]
    lam1, lam2 = c['lams'][0]
    xo, _ = reference(c['lams'][0])
    s = N.scale_of(y)
    seen = 0
    for rows, A in groups:
        x = xo[rows]
        assert N.kkt_ok(A, y[rows], x, lam1, lam2)[0].all()
        has = (x > 0).any(axis=1)
        seen += int(has.sum())
        # one support atom (the largest) zeroed
        bad = x.copy()
        bad[np.arange(len(x)), x.argmax(axis=1)] = 0.0
        assert not N.kkt_ok(A, y[rows], bad, lam1, lam2)[0][has].any()
        # all of x scaled by 1 + 1e-6
        assert not N.kkt_ok(A, y[rows], x * (1.0 + 1e-6), lam1, lam2)[0][has].any()
        # one clamped atom (the first) set to 1e-7 max|y|
        clamped = (x == 0).any(axis=1) & (s[rows] > 0)
        bad = x.copy()
        bad[np.arange(len(x)), (x == 0).argmax(axis=1)] = np.where(clamped, 1e-7 * s[rows], x[np.arange(len(x)), (x == 0).argmax(axis=1)])
        assert not N.kkt_ok(A, y[rows], bad, lam1, lam2)[0][clamped].any()
        # ... and an all-zero voxel with anything but zeros
        zero = s[rows] == 0
        bad = x.copy()
        bad[zero, 0] = 1e-300
        assert not N.kkt_ok(A, y[rows], bad, lam1, lam2)[0][zero].any()
    assert seen > N_VOX // 2
