"""Rician debias on the GPU (amx_debias_rows*, amx_prep_debias*; core.py:201-206 -> preproc.py:23-36).

The kernels compute the exact minimiser of the reference's separable functional, so the tests check optimality directly
(tests/debias_np.py: scipy's `ive` in float64, an independent evaluation of mu) and meet the reference through its objective value
and through the distance it stops at (tests/golden/debias_fixture.npz, made by tests/golden/make_debias_fixture.py).
Bounds: |mu(E) - S| <= 1e-10 S (Newton in fp64 ends within a few ulp; 1e-10 sits five orders above that and five below the reference's
stopping gap) and |E - exact| <= 1e-9 b0 where S >= 1.05 floor (there the root is well conditioned: mu' >= 0.29).  On the 100 000
synthetic voxels the residual bound is asserted on every sample; the comparison with an independently computed minimiser is a sample of
them (brentq on 40 voxels, a vectorised bisection on 10 000: scipy's ive on all 9.9 M samples, 64 times over, takes minutes)."""
import numpy as np
import pytest

import debias_np as D
from conftest import load_npz
from test_debias import fixture_rows
from amico_amd import synthetic as S

pytestmark = pytest.mark.gpu
CAP = 1e-4          # the project's bar on the maps (BASELINE.json)


def ctx():
    from amico_amd import get_context
    return get_context()


def check_optimal(E, rows, sigma, tag):
    rows64 = np.asarray(rows, dtype=np.float64)
    fl = D.floor_of(sigma)[:, None]
    below = rows64 <= fl
    assert not E[below].any(), tag
    res = np.abs(D.mu(E, sigma[:, None]) - rows64)
    worst = float(np.max(np.where(below, 0.0, res / np.where(below, 1.0, rows64))))
    print(f'{tag}: {int(below.sum())} of {below.size} samples at or below the floor, largest |mu(E) - S| / S above it {worst:.3e}')
    assert worst <= 1e-10, tag
    assert np.isfinite(E).all() and (E >= 0).all() and (E <= np.abs(rows64)).all(), tag
    return below


def synthetic_rows(n, seed=11):
    rng = np.random.default_rng(seed)
    nS, b0_idx = 99, np.arange(0, 99, 11, dtype=np.int32)
    snr = np.exp(rng.uniform(np.log(2.0), np.log(1000.0), size=n))
    amp = rng.uniform(50.0, 3000.0, size=n)
    att = rng.uniform(0.0, 1.0, size=(n, nS)) ** 2
    att[:, b0_idx] = 1.0
    sg = (amp / snr)[:, None]
    rows = np.abs(amp[:, None] * att + sg * rng.standard_normal((n, nS)) + 1j * sg * rng.standard_normal((n, nS))).astype(np.float32)
    return rows, b0_idx, snr


def test_rows_are_the_exact_minimiser_fixture_and_synthetic():
    from amico_amd import _capi
    c = ctx()
    f, rows, lvl, sigma = fixture_rows()
    E = np.empty(rows.shape)
    for k, snr in enumerate(f['snr_levels']):
        E[lvl == k] = _capi.debias_rows(c, rows[lvl == k], f['b0_idx'], float(snr))
        assert c.debias_last_unconverged() == 0
    below = check_optimal(E, rows, sigma, 'fixture')
    b0 = (sigma * f['snr_levels'][lvl])[:, None]
    well = rows >= 1.05 * D.floor_of(sigma)[:, None]
    d = np.abs(E - f['exact_E']) / np.abs(b0)
    print(f'fixture: largest |E - exact| / b0 where S >= 1.05 floor {d[well].max():.3e}, anywhere {d.max():.3e}')
    assert d[well].max() <= 1e-9
    # 100 000 synthetic voxels, SNR 2 .. 1000: a call takes one SNR, so the voxels' SNRs are whole numbers and each gets a call
    rows_s, b0_idx, snr = synthetic_rows(100000)
    snr_q = np.round(snr, 0)
    bins = np.unique(snr_q)
    E_s = np.empty(rows_s.shape)
    for v in bins:
        sel = snr_q == v
        E_s[sel] = _capi.debias_rows(c, rows_s[sel], b0_idx, float(v))
        assert c.debias_last_unconverged() == 0
    sigma_s = D.sigma_of(rows_s, b0_idx, 1.0) / snr_q
    check_optimal(E_s, rows_s, sigma_s, 'synthetic')
    pick = np.random.default_rng(0).choice(len(rows_s), 40, replace=False)
    ex = D.exact_minimiser(rows_s[pick], sigma_s[pick])
    well = rows_s[pick] >= 1.05 * D.floor_of(sigma_s[pick])[:, None]
    d = np.abs(E_s[pick] - ex) / np.abs(sigma_s[pick] * snr_q[pick])[:, None]
    print(f'synthetic (40 voxels against brentq): largest |E - exact| / b0 where S >= 1.05 floor {d[well].max():.3e}')
    assert d[well].max() <= 1e-9
    pick = np.arange(0, len(rows_s), 10)
    ex = D.bisect_minimiser(rows_s[pick], sigma_s[pick])
    well = rows_s[pick] >= 1.05 * D.floor_of(sigma_s[pick])[:, None]
    d = np.abs(E_s[pick] - ex) / np.abs(sigma_s[pick] * snr_q[pick])[:, None]
    print(f'synthetic (10 000 voxels against bisection): largest |E - exact| / b0 where S >= 1.05 floor {d[well].max():.3e}')
    assert d[well].max() <= 1e-9


def test_against_the_reference_objective_and_stopping_gap():
    from amico_amd import _capi
    c = ctx()
    f, rows, lvl, sigma = fixture_rows()
    E = np.empty(rows.shape)
    for k, snr in enumerate(f['snr_levels']):
        E[lvl == k] = _capi.debias_rows(c, rows[lvl == k], f['b0_idx'], float(snr))
    F_dev = D.objective(E, rows, sigma)
    print('F(device) / F(reference) - 1: max', float(np.max(F_dev / f['ref_F'] - 1.0)))
    assert (F_dev <= f['ref_F'] * (1.0 + 1e-12)).all()
    b0 = np.abs(sigma * f['snr_levels'][lvl])[:, None]
    for k, snr in enumerate(f['snr_levels']):
        g = float(np.max(np.abs(E - f['ref_E'])[lvl == k] / b0[lvl == k]))
        print(f'SNR {snr:g}: max |E - ref| / b0 = {g:.6e}, the exact minimiser\'s own gap {f["gap"][k]:.6e}')
        assert g <= f['gap'][k] + 1e-9


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_extremes(dtype):
    from amico_amd import _capi
    c = ctx()
    rng = np.random.default_rng(3)
    nS, b0_idx = 24, np.array([0, 7, 15], dtype=np.int32)
    base = rng.uniform(0.0, 1200.0, size=(64, nS))
    base[:, b0_idx] = rng.uniform(900.0, 1100.0, size=(64, 3))
    base[0, 3] = 0.0
    base[1, 4] = -35.0
    base[2, b0_idx] = -base[2, b0_idx]                        # negative b0 mean: acts like its absolute value
    base[3, b0_idx] = [5.0, -2.0, -3.0]                       # b0 mean exactly 0: unchanged
    base = base.astype(dtype)
    for snr in (0.5, 30.0, 1e5):
        rows = base.copy()
        sig = D.sigma_of(rows, b0_idx, snr)
        fl = D.floor_of(sig).astype(dtype).astype(np.float64)
        rows[5:9, 5] = fl[5:9].astype(dtype)                  # at the floor to the last bit of the input type
        rows[9, 5] = np.nextafter(dtype(fl[9]), dtype(np.inf))
        sig = D.sigma_of(rows, b0_idx, snr)
        assert sig[3] == 0.0 and sig[2] < 0
        E = _capi.debias_rows(c, rows, b0_idx, snr)
        assert c.debias_last_unconverged() == 0
        assert np.array_equal(E[3], rows[3].astype(np.float64))
        keep = np.arange(64) != 3
        check_optimal(E[keep], rows[keep], sig[keep], f'extremes {np.dtype(dtype).name} snr {snr:g}')
        assert E[0, 3] == 0.0 and E[1, 4] == 0.0
        at = rows[5:9, 5].astype(np.float64) <= D.floor_of(sig[5:9])
        assert np.array_equal(E[5:9, 5] == 0.0, at)
        # E scales with S at fixed SNR (powers of two: exact in both precisions)
        for scale in (2.0 ** -10, 2.0 ** 14):
            Es = _capi.debias_rows(c, (rows * dtype(scale)).astype(dtype), b0_idx, snr)
            assert np.isfinite(Es).all()
            assert np.array_equal(Es, E * scale)


@pytest.mark.parametrize('order', ['C', 'F'])
def test_image_form_in_place(order):
    import torch
    from amico_amd import prep
    f, rows, lvl, sigma = fixture_rows()
    sch = S.SimpleScheme(np.column_stack([np.tile([1.0, 0.0, 0.0], (99, 1)), np.where(np.isin(np.arange(99), f['b0_idx']), 0.0, 1000.0)]))
    assert np.array_equal(sch.b0_idx, f['b0_idx'])
    img0 = np.asarray(f['img'], order=order)
    for k, snr in enumerate(f['snr_levels']):
        sub = np.where(f['region'] == k, f['mask'], 0).astype(np.uint8)
        sp = prep.SignalPreparation(sch, img0, sub, do_normalize=False, debias_snr=float(snr))
        out = sp.debias(img0)
        assert out is not img0 and out.strides == img0.strides and sp.ctx.debias_last_unconverged() == 0
        assert not out[sub == 0].any()
        want = f['exact_E'][lvl == k].astype(np.float32)
        got = out[sub != 0]
        ulp = np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        # device entry on a buffer of its own: the same bits
        flat = np.array(sp._plan._img_buffer(img0))
        d = torch.from_numpy(flat).to('cuda')
        sp._plan.debias_device(d.data_ptr(), float(snr))
        sp.ctx.sync()
        back = np.lib.stride_tricks.as_strided(d.cpu().numpy(), shape=img0.shape, strides=img0.strides)
        assert np.array_equal(back, out)


def debiased_image_np(img, mask, b0_idx, snr):
    """numpy chain: exact minimiser (tests/debias_np.py) -> float32, zero outside mask != 0"""
    sel = mask != 0
    rows = img[sel]
    out = np.zeros(img.shape, dtype=np.float32)
    out[sel] = D.exact_minimiser(rows, D.sigma_of(rows, b0_idx, snr)).astype(np.float32)
    return np.asarray(out, order='F' if np.isfortran(img) else 'C')


def noisy_volume(y, shape, amp, snr, seed):
    rng = np.random.default_rng(seed)
    clean = y.reshape(shape + (-1,)) * amp
    sg = amp / snr
    return np.abs(clean + sg * rng.standard_normal(clean.shape) + 1j * sg * rng.standard_normal(clean.shape)).astype(np.float32)


@pytest.mark.parametrize('case', ['plain', 'b0_min_signal', 'doMergeB0', 'doDirectionalAverage'])
def test_pipeline(case, htable500):
    """Evaluation with doDebiasSignal: y is what the existing preparation makes of the debiased image, the maps follow the oracle's fit
    of the numpy chain exact -> float32 -> numpy preparation, and they differ from the maps with the flag off, which are untouched"""
    import amico_amd
    from amico_amd import prep
    from oracle import oracle, signal_np
    ht, snr = htable500['htable'], 12.0
    shape = (6, 5, 4)
    n = int(np.prod(shape))
    mask = np.random.default_rng(1).choice(np.array([0, 1, 1, 1, 2], dtype=np.uint8), size=shape)
    opts, b0min = {}, 0
    if case == 'doDirectionalAverage':
        sch = S.make_sandi_scheme(ndir_per_shell=12, n_b0=4)
        avg = S.directional_average_scheme(sch)
        K, Rs, d_in, d_isos = S.sandi_kernels(avg)
        ya = S.sandi_signals(n, K, avg, seed=3)
        y = np.ones((n, sch.nS))
        for k, sh in enumerate(sorted(sch.shells, key=lambda s: s['b'])):
            y[:, sh['idx']] = ya[:, k + 1][:, None]
        model, opts = 'SANDI', dict(do_directional_average=True)
    elif case == 'doMergeB0':
        sch = S.make_scheme(3, ((1000.0, 40),), seed=3)
        K = S.freewater_kernels(sch, htable500['dirs'])
        y, _ = S.freewater_signals(n, K, ht, sch, seed=2)
        model, opts = 'FreeWater', dict(do_merge_b0=True)
    else:
        sch = S.make_scheme(seed=0)
        K = S.noddi_kernels(sch, htable500['dirs'])
        y, _ = S.noddi_signals(n, K, ht, sch, seed=4)
        model = 'NODDI'
        b0min = 0.9 if case == 'b0_min_signal' else 0
    img = np.asfortranarray(noisy_volume(y, shape, 900.0, snr, seed=5))
    if case == 'b0_min_signal':
        img[:2] *= np.float32(0.5)                             # some voxels under 0.9 x the mean b0

    def run(debias):
        ae = amico_amd.Evaluation()
        for key in ('doMergeB0', 'doDirectionalAverage'):
            ae.set_config(key, case == key)
        if debias:
            ae.set_config('doDebiasSignal', True)
            ae.set_config('DWI-SNR', snr)
        ae.set_data(img, sch, mask, b0_min_signal=b0min)
        ae.set_model(model)
        if model == 'SANDI':
            ae.set_kernels(S.sandi_kernels(ae.scheme)[0])
        elif model == 'FreeWater':
            cols = np.hstack((sch.b0_idx[0], sch.dwi_idx))
            ae.set_kernels({'model': 'FreeWater', 'D': np.ascontiguousarray(K['D'][..., cols]), 'CSF': np.ascontiguousarray(K['CSF'][..., cols])}, ht)
        else:
            ae.set_kernels(K, ht)
        ae.fit()
        return ae

    off, on = run(False), run(True)
    assert on.get_config('debias_unconverged') == 0
    # flag off: the untouched path -- the preparation and a second Evaluation give the same bits
    sp0 = prep.SignalPreparation(sch, img, mask, b0_min_signal=b0min, **opts)
    assert np.array_equal(off.y, sp0.gather(img)[0])
    off2 = run(False)
    assert np.array_equal(off.y, off2.y) and np.array_equal(off.RESULTS['MAPs'], off2.RESULTS['MAPs'])
    # ... and its maps are the model's own fit of those signals (numpy in / numpy out, nothing of Evaluation.fit in between), to the
    # project's parity bar between two of its paths (1e-6, tests/test_gpu_parity.py: TOL) before the float32 volumes round them
    class Holder:
        y, DIRs, htable, KERNELS, nthreads = sp0.gather(img)[0], off.DIRs, off.htable, off.KERNELS, 4

        def get_config(self, k):
            return off.get_config(k) if k in ('doMergeB0', 'doDirectionalAverage', 'solver_params') else False
    own = off.model.fit(Holder())['estimates']
    d_own = np.abs(off.RESULTS['MAPs'][mask == 1] - own.astype(np.float32)).max()
    print(f'{case}: flag off, max |map - model.fit(prepared y)| {d_own:.3e}')
    assert d_own <= 1e-6
    # flag on: same kernels downstream of the debias entry
    deb = prep.SignalPreparation(sch, img, mask, do_normalize=False, debias_snr=snr).debias(img)
    assert np.array_equal(on.y, sp0.gather(deb)[0])
    # ... and the numpy chain
    deb_np = debiased_image_np(img, mask, sch.b0_idx, snr)
    one_ulp = np.abs(deb.astype(np.float64) - deb_np.astype(np.float64)) <= np.spacing(np.maximum(np.abs(deb_np), np.float32(1e-30)))
    assert one_ulp.all() and not deb[mask == 0].any()
    y_np, _ = signal_np.prepare_signal(deb, mask, sch.b0_idx, sch.dwi_idx, shells=sch.shells if case == 'doDirectionalAverage' else None,
                                       b0_min_signal=b0min, **opts)
    assert np.array_equal(on.y, y_np)
    y_np, _ = signal_np.prepare_signal(deb_np, mask, sch.b0_idx, sch.dwi_idx, shells=sch.shells if case == 'doDirectionalAverage' else None,
                                       b0_min_signal=b0min, **opts)
    sel = mask == 1
    if model == 'NODDI':
        ref = oracle.noddi_fit(y_np, on.DIRs, K, ht, sch.dwi_idx, nthreads=8)
    elif model == 'SANDI':
        ref = oracle.sandi_fit(y_np, S.sandi_kernels(on.scheme)[0], Rs, d_in, d_isos)
    else:
        ref = oracle.freewater_fit(y_np, on.DIRs, on.KERNELS, ht)
    diff = np.abs(on.RESULTS['MAPs'][sel] - ref['estimates'].astype(np.float32))
    print(f'{case}: max |map - oracle| {diff.max():.3e}; max |map on - map off| {np.abs(on.RESULTS["MAPs"] - off.RESULTS["MAPs"]).max():.3e}')
    assert diff.max() < CAP
    assert not np.array_equal(on.RESULTS['MAPs'], off.RESULTS['MAPs']) and not np.array_equal(on.y, off.y)


def test_volume_pipeline_with_debias(htable500):
    """NoddiVolumePipeline(debias_snr=...): the maps Evaluation gives with doDebiasSignal, bit for bit, and the caller's image buffer
    holds the debiased image afterwards"""
    import torch
    import amico_amd
    from amico_amd import pipeline, prep
    ht, snr = htable500['htable'], 15.0
    sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, htable500['dirs'])
    shape = (10, 8, 5)
    y, _ = S.noddi_signals(int(np.prod(shape)), K, ht, sch, seed=8)
    img = np.asfortranarray(noisy_volume(y, shape, 700.0, snr, seed=9))
    mask = np.random.default_rng(3).choice(np.array([0, 1, 1, 1, 2], dtype=np.uint8), size=shape)
    pl = pipeline.NoddiVolumePipeline(sch, img, mask, K, ht, debias_snr=snr)
    flat = np.lib.stride_tricks.as_strided(img, shape=(img.size,), strides=(4,))
    d_img = torch.from_numpy(flat.copy()).to('cuda:0')
    maps, dirs = pl.run(d_img)
    assert pl.ctx.debias_last_unconverged() == 0
    ae = amico_amd.Evaluation()
    ae.set_config('doDebiasSignal', True)
    ae.set_config('DWI-SNR', snr)
    ae.set_data(img, sch, mask)
    ae.set_model('NODDI')
    ae.set_kernels(K, ht)
    ae.fit()
    assert np.array_equal(maps.cpu().numpy(), ae.RESULTS['MAPs']) and np.array_equal(dirs.cpu().numpy(), ae.RESULTS['DIRs'])
    deb = prep.SignalPreparation(sch, img, mask, do_normalize=False, debias_snr=snr).debias(img)
    back = np.lib.stride_tricks.as_strided(d_img.cpu().numpy(), shape=img.shape, strides=img.strides)
    assert np.array_equal(back, deb) and not back[mask == 0].any()
    plain = pipeline.NoddiVolumePipeline(sch, img, mask, K, ht)
    maps0, _ = plain.run(torch.from_numpy(flat.copy()).to('cuda:0'))
    assert not np.array_equal(maps0.cpu().numpy(), maps.cpu().numpy())
