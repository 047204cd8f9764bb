"""SANDI on protocols of 129 .. 512 volumes (no directional average): k_sandi_project (c = A'y, y'y on the fp64 matrix cores) ->
k_sandi_gram_lane<N> (<= 16 atoms) or k_sandi_gram_wave, against the CPU oracle on the same inputs.

Shapes: 129 volumes is the first past the old cap -- odd, so the K tail is one sample and float32 rows (516 bytes) are not 16-byte
aligned; 306 is the default acquisition; 512 the bound.  12 / 15 / 16 atoms are the lane kernel's three instantiations, 13 has padding
atoms inside N = 15, 24 takes two atom tiles and the wavefront kernel.  1 / 17 / 65 / 1 029 voxels are the tails of the 16-voxel MFMA
group and of the 64-voxel hand-over block.  tests/test_sandi_long.py pins the oracle these tests compare with.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-6           # the project's bound on maps and error maps against the oracle (tests/test_gpu_parity.py)
W_P_TOL = 1e-9       # |dual value| on the support, largest admissible dual value off it (tests/test_gpu_kkt.py, the ridge models)
W_Z_TOL = 1e-9

SCHEMES = {129: dict(ndir_per_shell=25, n_b0=4), 306: {}, 512: dict(ndir_per_shell=100, n_b0=12), 513: dict(ndir_per_shell=100, n_b0=13),
           100: dict(ndir_per_shell=19, n_b0=5)}
ATOMS = {15: (5, 5, 5), 12: (4, 4, 4), 13: (5, 4, 4), 16: (5, 5, 6), 24: (8, 8, 8)}
NEW_KERNELS = ('k_sandi_project', 'k_sandi_gram')


class Holder:
    def __init__(self, y, kernels, **cfg):
        self.y, self.DIRs, self.htable, self.KERNELS, self.nthreads = y, None, None, kernels, 4
        self._cfg = cfg

    def get_config(self, k):
        return self._cfg.get(k, False)


@functools.lru_cache(maxsize=None)
def _dictionary(nS, n_atoms=15):
    from amico_amd import synthetic as S
    sch = S.make_sandi_scheme(**SCHEMES[nS])
    assert sch.nS == nS
    a, b, c = ATOMS[n_atoms]
    K, Rs, d_in, d_isos = S.sandi_kernels(sch, Rs=np.linspace(1.0, 12.0, a) * 1e-6, d_in=np.linspace(0.25, 3.0, b) * 1e-3,
                                          d_isos=np.linspace(0.25, 3.0, c) * 1e-3)
    return sch, K, Rs, d_in, d_isos


@functools.lru_cache(maxsize=None)
def _case(nS, n_atoms, n_vox, lam1, lam2):
    """signals and the oracle's fit of them, computed once and shared (read-only)"""
    from amico_amd import synthetic as S
    from oracle import oracle
    sch, K, Rs, d_in, d_isos = _dictionary(nS, n_atoms)
    y = S.sandi_signals(n_vox, K, sch, seed=3, navg=1)
    ref = oracle.sandi_fit(y, K, Rs, d_in, d_isos, lam1, lam2, rmse=True, nrmse=True, return_x=True)
    y.setflags(write=False)
    return y, ref


def _upload(ctx, nS, n_atoms=15):
    from amico_amd import _capi
    _, K, Rs, d_in, d_isos = _dictionary(nS, n_atoms)
    return _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)


def _fit(ctx, lut, y, lam1, lam2, **kw):
    """device fit of host rows -> numpy (estimates, rmse, nrmse[, x])"""
    import torch
    from amico_amd import _capi
    out = _capi.sandi_fit_device(ctx, lut, torch.from_numpy(np.array(y)).cuda(), lam1, lam2, rmse=True, nrmse=True, **kw)
    ctx.sync()
    return tuple(t.cpu().numpy() for t in out)


CASES = [(129, 15, 1029, 0.0, 5e-3), (306, 15, 1029, 0.0, 5e-3), (512, 15, 1029, 0.0, 5e-3),
         (306, 12, 1029, 0.0, 5e-3), (306, 13, 1029, 0.0, 5e-3), (306, 16, 1029, 0.0, 5e-3), (306, 24, 1029, 0.0, 5e-3),
         (129, 15, 1, 0.0, 5e-3), (129, 15, 17, 0.0, 5e-3), (129, 15, 65, 0.0, 5e-3), (129, 24, 17, 0.0, 5e-3), (512, 24, 65, 0.0, 5e-3),
         (306, 15, 1029, 0.05, 5e-3), (306, 15, 1029, 0.0, 1e-4), (129, 16, 65, 0.05, 5e-3),
         (306, 24, 1029, 0.05, 5e-3), (306, 24, 1029, 0.0, 1e-4)]


@pytest.mark.parametrize('nS,n_atoms,n_vox,lam1,lam2', CASES)
def test_long_protocol_against_the_oracle(nS, n_atoms, n_vox, lam1, lam2):
    """every voxel: six maps, rmse, nrmse within TOL of the oracle; the device x is the optimum of the full problem (KKT in numpy)"""
    from amico_amd import get_context
    y, ref = _case(nS, n_atoms, n_vox, lam1, lam2)
    _, K, _, _, _ = _dictionary(nS, n_atoms)
    ctx = get_context()
    lut = _upload(ctx, nS, n_atoms)
    est, rmse, nrmse, xd = _fit(ctx, lut, y, lam1, lam2, return_x=True)
    path, st = ctx.last_path(), ctx.last_stats()
    lut.close()
    d_est, d_rmse, d_nrmse = np.abs(est - ref['estimates']).max(), np.abs(rmse - ref['rmse']).max(), np.abs(nrmse - ref['nrmse']).max()
    x = xd / K['norms'][None, :]                               # undo models.pyx:1570-1571 for the certificate
    A = np.asarray(K['signal'], dtype=np.float64)
    g = y @ A - x @ (A.T @ A + lam2 * np.eye(n_atoms)) - lam1
    P = x > 0
    gp, gz = float(np.abs(g[P]).max(initial=0.0)), float(g[~P].max(initial=0.0))
    print(f'{nS} x {n_atoms}, {n_vox} voxels, lambda ({lam1}, {lam2}) [{path}]: max |maps - oracle| {d_est:.3e}, rmse {d_rmse:.3e}, '
          f'nrmse {d_nrmse:.3e}, |g_P| {gp:.3e}, max g_Z {gz:.3e}, mean rmse {rmse.mean():.3f}, {st}')
    assert 'k_sandi_project<double>' in path and ('k_sandi_gram_lane<%d>' % {12: 12, 13: 15, 15: 15, 16: 16}[n_atoms] if n_atoms <= 16 else 'k_sandi_gram_wave') in path
    assert est.shape == (n_vox, 6) and np.isfinite(est).all() and np.isfinite(rmse).all() and np.isfinite(nrmse).all()
    assert d_est < TOL and d_rmse < TOL and d_nrmse < TOL
    assert st['itercap_voxels'] == 0 and st['guard_trips'] == 0 and st['overflow_voxels'] == 0
    assert x.min() >= 0.0 and gp < W_P_TOL and gz < W_Z_TOL


def test_lane_and_wave_routes_agree(amx_env):
    from amico_amd import get_context
    y, _ = _case(306, 15, 1029, 0.0, 5e-3)
    ctx = get_context()
    lut = _upload(ctx, 306)
    lane = _fit(ctx, lut, y, 0.0, 5e-3, return_x=True)
    assert 'k_sandi_gram_lane<15>' in ctx.last_path()
    lut.close()
    amx_env(AMX_WAVE_PER_VOXEL='1')
    ctx = get_context()
    lut = _upload(ctx, 306)
    wave = _fit(ctx, lut, y, 0.0, 5e-3, return_x=True)
    assert 'k_sandi_gram_wave' in ctx.last_path() and 'k_sandi_gram_lane' not in ctx.last_path()
    assert ctx.last_stats()['itercap_voxels'] == 0 and ctx.last_stats()['guard_trips'] == 0
    lut.close()
    for a, b, what in zip(lane, wave, ('maps', 'rmse', 'nrmse', 'x')):
        d = np.abs(a - b).max()
        print(f'lane against wave, {what}: {d:.3e}')
        assert d < 1e-9, what


def test_float32_device_signals_and_float64_host_path_agree():
    """float32 rows of 129 samples (516 bytes: aligned to 4 only) are read in place; the same values as float64 through the host call"""
    import torch
    from amico_amd import SANDI, _capi, get_context
    y, _ = _case(129, 15, 1029, 0.0, 5e-3)
    y32 = y.astype(np.float32)
    _, K, Rs, d_in, d_isos = _dictionary(129)
    ctx = get_context()
    lut = _upload(ctx, 129)
    out = _capi.sandi_fit_device(ctx, lut, torch.from_numpy(y32).cuda(), 0.0, 5e-3, rmse=True, nrmse=True)
    ctx.sync()
    assert 'k_sandi_project<float>' in ctx.last_path(), ctx.last_path()      # (no float64 copy of y first)
    lut.close()
    est, rmse, nrmse = (t.cpu().numpy() for t in out)
    host = SANDI().fit(Holder(y32.astype(np.float64), K, doComputeRMSE=True, doComputeNRMSE=True))
    d = np.abs(host['estimates'] - est).max(), np.abs(host['rmse'] - rmse).max(), np.abs(host['nrmse'] - nrmse).max()
    print('float32 device against float64 host: maps %.3e, rmse %.3e, nrmse %.3e' % d)
    assert max(d) < 1e-12


@pytest.mark.parametrize('route', ['lane', 'wave'])
def test_bad_samples_give_nan_and_touch_nobody_else(route, amx_env):
    from amico_amd import get_context
    if route == 'wave':
        amx_env(AMX_WAVE_PER_VOXEL='1')
    y, _ = _case(129, 15, 65, 0.0, 5e-3)
    bad = y.copy()
    bad[3, 7] = np.nan              # both share their 16-voxel group with good voxels; 128 is the sample of the K tail
    bad[20, 128] = np.inf
    ctx = get_context()
    lut = _upload(ctx, 129)
    clean = _fit(ctx, lut, y, 0.0, 5e-3)
    dirty = _fit(ctx, lut, bad, 0.0, 5e-3)
    assert ctx.last_stats()['itercap_voxels'] == 0 and ctx.last_stats()['guard_trips'] == 0
    lut.close()
    good = np.ones(65, dtype=bool)
    good[[3, 20]] = False
    for a, b in zip(clean, dirty):
        assert np.isnan(b[~good]).all()
        assert np.isfinite(a).all() and np.array_equal(a[good], b[good])      # to the last bit


@pytest.mark.parametrize('factor', [2.0 ** -10, 2.0 ** 14])
def test_amplitude(factor):
    from amico_amd import get_context
    y, _ = _case(306, 15, 1029, 0.0, 5e-3)
    ctx = get_context()
    lut = _upload(ctx, 306)
    unit = _fit(ctx, lut, y, 0.0, 5e-3)
    scaled = _fit(ctx, lut, y * factor, 0.0, 5e-3)
    lut.close()
    print('amplitude %g: maps %.3e, rmse / factor %.3e, nrmse %.3e' % (factor, np.abs(scaled[0] - unit[0]).max(),
                                                                        np.abs(scaled[1] / factor - unit[1]).max(), np.abs(scaled[2] - unit[2]).max()))
    assert np.abs(scaled[0] - unit[0]).max() < TOL
    assert np.abs(scaled[1] / factor - unit[1]).max() < TOL      # rmse scales with the signal, nrmse does not
    assert np.abs(scaled[2] - unit[2]).max() < TOL


def test_routing():
    """the new kernels run past 128 volumes only; shorter protocols keep their kernels"""
    from amico_amd import get_context, synthetic as S
    ctx = get_context()
    y, _ = _case(129, 15, 65, 0.0, 5e-3)
    lut = _upload(ctx, 129)
    _fit(ctx, lut, y, 0.0, 5e-3)
    path = ctx.last_path()
    lut.close()
    assert 'k_sandi_project' in path and 'k_sandi_gram_lane<15>' in path, path
    for nS in (6, 100):
        sch = S.directional_average_scheme(S.make_sandi_scheme()) if nS == 6 else S.make_sandi_scheme(**SCHEMES[100])
        assert sch.nS == nS
        K, Rs, d_in, d_isos = S.sandi_kernels(sch)
        ys = S.sandi_signals(65, K, sch, seed=3, navg=60 if nS == 6 else 1)
        from amico_amd import _capi
        lut = _capi.upload_sandi(ctx, K, Rs, d_in, d_isos)
        _fit(ctx, lut, ys, 0.0, 5e-3)
        path = ctx.last_path()
        lut.close()
        assert path and not any(k in path for k in NEW_KERNELS), path


def test_513_volumes_are_refused_at_upload():
    from amico_amd import get_context
    with pytest.raises(ValueError, match='512'):
        _upload(get_context(), 513)


def test_no_ridge_is_refused_past_128_volumes():
    """lambda2 = 0: an isotropic dictionary has rank <= shells + 1 < n_atoms -- no unique optimum, no Gram route"""
    from amico_amd import SANDI
    y, _ = _case(129, 15, 65, 0.0, 5e-3)
    _, K, _, _, _ = _dictionary(129)
    m = SANDI()
    m.set_solver(lambda1=0.0, lambda2=0.0)
    with pytest.raises(ValueError, match='more than 128 volumes need lambda2 >= 1e-9'):
        m.fit(Holder(np.array(y), K))


def test_evaluation_without_directional_average():
    """raw image 6 x 5 x 4 x 129, partly masked -> prepared signals, directions, SANDI fit, volumes -- doDirectionalAverage at its default (off)"""
    import amico_amd
    from amico_amd import synthetic as S
    from oracle import oracle, signal_np
    full, K, Rs, d_in, d_isos = _dictionary(129)
    shape = (6, 5, 4)
    n = int(np.prod(shape))
    ys = S.sandi_signals(n, K, full, seed=11, navg=1)
    img = np.asfortranarray((1000.0 * ys.reshape(shape + (-1,))).astype(np.float32))
    mask = np.ones(shape, dtype=np.uint8)
    mask[0, :, :] = 0
    mask[3, 2, 1] = 0
    sel = mask == 1
    ae = amico_amd.Evaluation()
    ae.set_config('doComputeNRMSE', True)
    ae.set_config('doSavePredictedSignal', True)
    ae.set_data(img, full, mask)
    assert ae.scheme.nS == 129
    ae.set_model('SANDI')
    ae.set_kernels(S.sandi_kernels(ae.scheme)[0])
    res = ae.fit()
    y_ref, mean_b0 = signal_np.prepare_signal(img, mask, full.b0_idx, full.dwi_idx)
    assert np.array_equal(ae.y, y_ref)
    ref = oracle.sandi_fit(y_ref, K, Rs, d_in, d_isos, nrmse=True, return_x=True)
    assert np.abs(res['estimates'] - ref['estimates']).max() < TOL
    assert ae.RESULTS['MAPs'].shape == shape + (6,) and not ae.RESULTS['MAPs'][~sel].any()
    assert np.abs(ae.RESULTS['MAPs'][sel] - ref['estimates']).max() < 1e-5       # (float32 volume: Rsoma is in micrometres)
    assert np.allclose(ae.RESULTS['NRMSE'][sel], ref['nrmse'], atol=TOL)
    # the reference computes directions whenever the average is off (core.py:456)
    assert ae.RESULTS['DIRs'].shape == shape + (3,) and ae.DIRs.shape == (int(sel.sum()), 3)
    # the predicted signal: the rescaled x on the normalised dictionary (the quirk the error maps share), times mean_b0
    pred = ref['x'] @ np.asarray(K['signal'], dtype=np.float64).T
    vol = ae.RESULTS['DWI_predicted']
    assert vol.dtype == np.float32 and vol.shape == shape + (129,) and not vol[~sel].any()
    assert np.abs(res['y_est'] - pred).max() < TOL
    m = mean_b0[sel].astype(np.float64)[:, None]
    assert np.abs(vol[sel] / m - pred).max() < TOL
