"""The numpy helpers of the CylinderZeppelinBall route tests (czb_np.py) against the golden fixture and the CPU oracle."""
import numpy as np

import czb_np as Z


def test_certificate_and_maps_of_the_fixture(czb_fix):
    f = czb_fix
    gp, gz, mn = Z.czb_certificate(f['kernels'], f['lut'], f['y'], f['x'], float(f['lambda1']), float(f['lambda2']))
    assert gp < 1e-10 and gz < 1e-10 and mn >= 0.0, (gp, gz, mn)
    maps = Z.czb_maps(f['x'], f['Rs'], len(f['d_perps']))                  # (the fixture sums voxel by voxel: rounding of the sums only)
    assert (np.abs(maps - f['estimates']) <= 1e-13 * np.abs(f['estimates'])).all()
    # a wrong coefficient does not pass: the certificate is not vacuous
    x = f['x'].copy()
    x[3, np.argmax(x[3])] *= 1.0 + 1e-8
    assert Z.czb_certificate(f['kernels'], f['lut'], f['y'], x, 0.0, 4.0)[0] > 1e-9


def test_dictionaries_are_the_fixture_construction(czb_fix, htable500):
    """czb_kernels on the fixture's scheme and orientations: the fixture's atoms, up to the 6e-7 by which this repository's cylinder
    response differs from the tabulated roots the fixture was generated with (amico_amd/synthesis.py)"""
    from amico_amd import synthetic as S
    f = czb_fix
    K = Z.czb_kernels(S.SimpleScheme(f['scheme']), f['lut_ids'], f['Rs'], f['d_perps'], f['d_isos'], 0.6e-3, lut_dirs=htable500['dirs'])
    for k in ('wmr', 'wmh', 'iso'):
        assert K[k].shape == f['kernels'][k].shape and K[k].dtype == np.float32
        assert np.abs(K[k].astype(np.float64) - f['kernels'][k]).max() < 2e-6, k
    b0 = S.SimpleScheme(f['scheme']).b0_idx
    assert (K['wmr'][:, f['lut_ids']][:, :, b0] == 1.0).all() and (K['iso'][:, b0] == 1.0).all()
    other = np.setdiff1d(np.arange(500), f['lut_ids'])
    assert not K['wmr'][:, other].any() and not K['wmh'][:, other].any()


def test_schemes_and_directions(htable500):
    from amico_amd import synthetic as S
    for nS, at in ((30, 'start'), (101, 'middle'), (160, 'single'), (512, 'middle')):
        sch = Z.make_scheme(nS, at)
        assert sch.nS == nS and sch.version == 1
        assert sch.b0_count == 1 if at == 'single' else sch.b0_count >= 2
        assert (sch.b0_idx[0] == 0) == (at != 'middle')
    rng = np.random.default_rng(0)
    ori = rng.integers(0, 500, 3000)
    d = Z.dirs_in_cells(ori, htable500['dirs'], htable500['htable'], rng)
    assert np.array_equal(S.lut_indices(d, htable500['htable']), ori)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-12


def test_oracle_supports_against_the_long_double_resolve(czb_fix, htable500):
    """the support comparison of test_gpu_czb_paths.py exempts atoms whose oracle coefficient or dual value lies below the bound
    2 sqrt(n) 1e-9 / lambda2 and lets at most 1e-4 of the voxels need that: here the oracle's supports against a re-solve with
    long-double residuals on standard and hard signals -- identical on every voxel, and the oracle's certificate within the 1e-9 the
    bound assumes"""
    from oracle import oracle
    f = czb_fix
    K, ids = f['kernels'], f['lut_ids']
    ht = htable500['htable']
    rng = np.random.default_rng(11)
    for hard, lam1 in ((False, 0.0), (True, 0.0), (True, 0.5)):
        n = 400
        lut = ids[rng.integers(len(ids), size=n)]
        y = Z.czb_signals(K, lut, rng, hard=hard)
        d = Z.dirs_in_cells(lut, htable500['dirs'], ht, rng)
        x = oracle.czb_fit(y, d, K, f['Rs'], ht, lam1, 4.0, nthreads=4, return_x=True)['x']
        gp, gz, mn = Z.czb_certificate(K, lut, y, x, lam1, 4.0)
        assert gp < 1e-9 and gz < 1e-9 and mn >= 0.0, (hard, lam1, gp, gz)
        bound = Z.x_bound(26, 4.0)
        g = Z.czb_gradient(K, lut, y, x, lam1, 4.0)
        need = 0
        for v in range(n):
            xr, gr = Z.czb_resolve(Z.dictionary(K, lut[v]), y[v], lam1, 4.0)
            assert np.abs(xr - x[v]).max() <= bound
            diff = (xr > 0) != (x[v] > 0)
            if diff.any():
                need += 1
                assert ((np.abs(x[v]) <= bound) & (np.abs(g[v]) <= bound))[diff].all(), (v, x[v][diff], g[v][diff])
        assert need / n < 1e-4, (hard, lam1, need)


def test_resolve_is_the_optimum():
    rng = np.random.default_rng(2)
    A = np.abs(rng.normal(size=(40, 12)))
    for lam1, lam2 in ((0.0, 4.0), (0.7, 0.5), (30.0, 4.0)):
        y = np.abs(rng.normal(size=40))
        x, g = Z.czb_resolve(A, y, lam1, lam2)
        gg = A.T @ (y - A @ x) - lam2 * x - lam1
        assert x.min() >= 0 and np.abs(gg[x > 0]).max(initial=0.0) < 1e-12 and gg[x == 0].max(initial=0.0) < 1e-12
        assert np.abs(g - gg)[x == 0].max(initial=0.0) < 1e-12
