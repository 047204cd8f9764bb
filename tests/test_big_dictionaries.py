"""The inputs of test_gpu_big_dictionaries.py are admissible: on every shape and ridge of big_np.CASES the CPU oracle alone passes the
per-voxel Kuhn-Tucker certificate the device is held to (small_np.kkt_ok: min x >= 0, max |g_P| < 1e-9 s, max g_Z < 1e-9 s with
s = max |y| of the voxel, long-double residual) on EVERY voxel, with err == 0.  With lambda1 = lambda2 = 0 the reference is the oracle's
A-space NNLS: its elastic net loses positive definiteness there."""
import numpy as np
import pytest

import big_np as B
import small_np as N


@pytest.mark.parametrize('name,lam', B.RUNS, ids=B.ids(B.RUNS))
def test_oracle_passes_the_certificate_on_every_voxel(name, lam):
    c = B.CASES[name]
    y, d, lut, kind = B.problem(name)
    assert len(y) == sum(c['counts']) and y.shape[1] == c['nS']
    if d is not None:
        assert sorted(np.bincount(lut)[B.ORI]) == sorted(c['counts'])
    # the mix holds its hard kinds: all-zero, one-atom, isotropic-only and pure-noise voxels
    assert {0, 1, 2, 3} <= set(kind.tolist())
    xo, mo = B.reference(name, lam)                      # (asserts err == 0 / mode == 1)
    assert xo.shape == (len(y), B.n_atoms_of(c)) and np.isfinite(xo).all() and np.isfinite(mo).all()
    ok, gp, gz = B.certificate(name, xo, lam)
    supp = (xo > 0).sum(axis=1)
    print('BIGDICT oracle %-16s (%g, %g)  gP/s %.2e  gZ/s %.2e  support mean %.0f max %d of %d' %
          (name, lam[0], lam[1], gp.max(), gz.max(), supp.mean(), supp.max(), xo.shape[1]))
    assert ok.all(), (name, lam, int((~ok).sum()), int(np.flatnonzero(~ok)[0]), float(gp.max()), float(gz.max()), sorted(set(N.KINDS[k] for k in kind[~ok])))
    # the maps the oracle reports are the model's arithmetic on its own coefficients
    assert np.abs(B.maps_of(name, xo) - mo).max() <= 1e-9 * max(1.0, np.abs(mo).max())


def test_shapes_cover_the_route():
    """the shapes the issue names are in the table"""
    na = {n: B.n_atoms_of(c) for n, c in B.CASES.items()}
    for model in ('fw', 'sandi', 'czb'):
        mine = [n for n, c in B.CASES.items() if c['model'] == model]
        assert any(na[n] == 65 for n in mine) and any(na[n] == 256 for n in mine) and any(na[n] == 64 and B.CASES[n]['small'] for n in mine)
        assert all((na[n] > 64) != B.CASES[n]['small'] for n in mine)
    assert na['fw_33x101'] == 101 and B.CASES['fw_512x256']['nS'] == 512 and B.CASES['fw_mouse_33x65']['mouse']
    assert {B.CASES[n]['nS'] for n in B.CASES if n.startswith('sandi') and na[n] == 90} == {100, 129}
    assert any(B.CASES[n]['nS'] < na[n] for n in B.CASES)


def test_a_small_pivot_has_its_digits_in_a_space_only():
    """the rule k_enet_big adds to the rank guard (amx_bpp.hpp, kSmall): on FreeWater 21 x 256 a zeppelin behind a few others lies
    within 1e-6 of their span.  Its Cholesky pivot in Gram space, H_jj - |l|^2, then has a digit or none (kPiv = 1e-13 drops the atom);
    evaluated as |a_j - A_P w|^2 from the dictionary it has three and more, down to its own floor -- and below that floor the value is
    noise, which the floor says"""
    A = B.matrix('fw_21x256', int(B.ORI[0]))
    tiny = noise = 0
    for P in ([100, 104, 102], [100, 110, 120, 105], [100, 120, 140, 110], [10, 60, 110, 160, 85], [100, 102, 104, 106, 103],
              [0, 50, 100, 150, 200, 250, 125], [100, 102, 104, 103], [100, 102, 104, 106, 108, 110, 106]):      # (the last: an atom that IS in the set)
        gram, aspace, exact, floor = B.pivots_of_last_atom(A, P)
        print('BIGDICT pivot / H_jj of zeppelin %3d behind %-28s Gram %.3e  A-space %.3e  long double %.3e  floor %.1e' % (P[-1], P[:-1], gram, aspace, exact, floor))
        if exact > 100 * floor:
            assert abs(aspace - exact) <= 1e-3 * exact, P
            if exact < 1e-14:
                tiny += 1
                assert abs(gram - exact) > 1e-2 * exact, P      # Gram space: not two digits
        elif exact < 1e-2 * floor:
            noise += 1
            assert aspace <= floor, P                            # what the evaluation gives is under the floor: the atom is dropped
    assert tiny >= 2 and noise >= 1
