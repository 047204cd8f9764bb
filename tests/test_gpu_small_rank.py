"""NODDI through the seeded chain (seed solvers -> Gram-space certificates -> left-over kernels) on dictionaries whose rank is below
the kSeedKD = 12 directions of the compressed basis: a small grid of atoms, and a protocol of fewer than 12 volumes.  The tables such a
dictionary gets are checked one by one in test_gpu_tables.py; here every voxel of a fit that reads them is held to the oracle.
test_lut.py fits a 3 x 3 grid as well, but on 3000 voxels -- below AMX_SEED_MIN_VOXELS, so the seeded chain never ran on one."""
import os

import numpy as np
import pytest

from kkt_certificates import noddi_certificates

pytestmark = pytest.mark.gpu

N_VOX = 4096
KKT_TOL = 1e-9       # W_P_TOL = W_Z_TOL of test_gpu_kkt.py
LIMIT = 1e-6         # maps and rmse against the oracle (test_gpu_parity.py)


def _fit(htable500, amx_env, sch, grid, seed):
    import torch
    amx_env(AMX_SEED_MIN_VOXELS='0')
    from amico_amd import _capi, get_context, synthetic as S
    from oracle import oracle
    dirs, ht = htable500['dirs'], htable500['htable']
    K = S.noddi_kernels(sch, dirs, **grid)
    y, d = S.noddi_signals(N_VOX, K, ht, sch, seed=seed, snr=20.0)
    ctx = get_context()
    lut = _capi.upload_noddi(ctx, K, ht, sch.dwi_idx)
    dev = torch.device('cuda', 0)
    est, rmse, _, _, xd = _capi.noddi_fit_device(ctx, lut, torch.from_numpy(y).to(dev), torch.from_numpy(d).to(dev), 0.5, 1e-3, 3,
                                                 rmse=True, return_x=True)
    ctx.sync()
    st, seeds = ctx.last_stats(), ctx.last_seed_stats()
    assert seeds['seeded_voxels'] == N_VOX, (seeds, ctx.last_path())
    assert st['itercap_voxels'] == 0 and st['guard_trips'] == 0 and st['overflow_voxels'] == 0, st
    ref = oracle.noddi_fit(y, d, K, ht, sch.dwi_idx, nthreads=os.cpu_count() or 1, rmse=True)
    print('seeded chain: %s' % seeds)
    return K, ht, y, d, est.cpu().numpy(), rmse.cpu().numpy(), xd.cpu().numpy(), ref


def test_ten_atoms_on_99_volumes(htable500, amx_env):
    """3 x 3 grid + iso: the optimum is unique, the maps of EVERY voxel are the oracle's"""
    from amico_amd import synthetic as S
    sch = S.make_scheme(seed=0)
    grid = dict(IC_VFs=np.linspace(0.1, 0.99, 3), IC_ODs=np.array([0.03, 0.5, 0.99]))
    K, ht, y, d, est, rmse, x, ref = _fit(htable500, amx_env, sch, grid, 31)
    assert K['wm'].shape[0] == 9 and sch.nS == 99
    diff = np.abs(est - ref['estimates']).max(axis=1)
    print('max |dmap| %.3e, max |drmse| %.3e' % (diff.max(), np.abs(rmse - ref['rmse']).max()))
    assert np.isfinite(est).all() and diff.max() < LIMIT, (diff.max(), int((diff >= LIMIT).sum()))
    assert np.abs(rmse - ref['rmse']).max() < LIMIT


def test_145_atoms_on_10_volumes(htable500, amx_env):
    """more atoms than volumes: x is not unique (neither x nor the maps are compared), A x is -- every voxel's coefficients pass the
    Kuhn-Tucker certificate of each stage, and every voxel's rmse is the oracle's"""
    from amico_amd import synthetic as S
    sch = S.make_scheme(n_b0=1, shells=((700.0, 4), (2000.0, 5)), seed=5)
    K, ht, y, d, est, rmse, x, ref = _fit(htable500, amx_env, sch, {}, 32)
    assert K['wm'].shape[0] == 144 and sch.nS == 10
    c = noddi_certificates(K, sch, ht, y, d, x, 0.5, 1e-3)
    print(c, 'max |drmse| %.3e' % np.abs(rmse - ref['rmse']).max())
    assert np.isfinite(x).all() and np.isfinite(rmse).all()
    assert c['min_x'] >= 0.0 and c['s3_off_support'] == 0.0, c
    assert c['s1_wP'] < KKT_TOL and c['s2_gP'] < KKT_TOL and c['s3_wP'] < KKT_TOL, c
    assert c['s1_wZ'] < KKT_TOL and c['s2_gZ'] < KKT_TOL and c['s3_wZ'] < KKT_TOL, c
    assert np.abs(rmse - ref['rmse']).max() < LIMIT, np.abs(rmse - ref['rmse']).max()
