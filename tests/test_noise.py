"""The noise estimate from the b0 repeats (amico_amd/noise.py, doEstimateNoise): what can be checked without a device --
the chi-square median ratio, that the estimator as restated in tests/noise_np.py recovers a known SNR and sigma from Rician samples,
and the configuration rules of Evaluation.set_data, which all act before anything is uploaded."""
import os
import re

import numpy as np
import pytest

import noise_np as N
from amico_amd import synthetic as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


@pytest.mark.parametrize('nu', [1, 2, 5, 9, 127])
def test_chi2_median_ratio(nu):
    from scipy import stats
    from amico_amd import noise
    want = stats.chi2.median(nu) / nu
    assert abs(noise.chi2_median_ratio(nu) - want) <= 1e-12 * want
    assert noise.chi2_median_ratio(nu) == N.chi2_median_ratio(nu)


def test_chi2_median_ratio_known_values():
    from amico_amd import noise
    assert abs(noise.chi2_median_ratio(1) - 0.45494) < 5e-6
    assert abs(noise.chi2_median_ratio(2) - np.log(2.0)) < 1e-14
    assert abs(noise.chi2_median_ratio(9) - 0.92698) < 5e-6
    with pytest.raises(ValueError):
        noise.chi2_median_ratio(0)


def rician_rows(n, k, snr, amp=1000.0, seed=7, nS=11):
    """n voxels whose k b0 repeats are Rician samples of amplitude `amp` at sigma = amp / snr, float32; the other columns attenuated"""
    rng = np.random.default_rng(seed)
    b0_idx = np.arange(k, dtype=np.int32)
    sg = amp / snr
    clean = np.full((n, nS), 0.4 * amp)
    clean[:, b0_idx] = amp
    rows = np.abs(clean + sg * rng.standard_normal((n, nS)) + 1j * sg * rng.standard_normal((n, nS))).astype(np.float32)
    return rows, b0_idx, sg


@pytest.mark.parametrize('snr', [10.0, 30.0])
@pytest.mark.parametrize('k', [2, 6])
def test_restatement_recovers_snr_and_sigma(k, snr):
    """Rician samples, 20 000 voxels, seed fixed: both estimates within 5 % of the truth (a trial of this estimator gave at most 1.8 %
    over 20 draws at this size: the scatter of a median over 20 000 voxels plus the Rician bias, +0.6 % at SNR 10)"""
    rows, b0_idx, sg = rician_rows(20000, k, snr)
    est = N.estimate(rows, b0_idx)
    print(f'k {k} SNR {snr}: SNR_est {est["snr"]:.4f} ({est["snr"] / snr - 1:+.2%}), sigma_est {est["sigma"]:.4f} ({est["sigma"] / sg - 1:+.2%}), '
          f'{est["voxels"]} voxels')
    assert est['voxels'] == 20000
    assert abs(est['snr'] / snr - 1.0) <= 0.05
    assert abs(est['sigma'] / sg - 1.0) <= 0.05


def test_restatement_marks_ineligible_voxels():
    rows = np.full((5, 4), 100.0)
    rows[:, 1] = 101.0
    rows[1, 0] = np.nan
    rows[2, 2] = np.inf
    rows[3, :] = 7.0                    # no spread
    rows[4, :3] = [-5.0, -6.0, -4.0]    # mean <= 0
    mean, sd, ratio = N.per_voxel(rows, [0, 1, 2])
    for a in (mean, sd, ratio):
        assert np.array_equal(np.isnan(a), [False, True, True, True, True])
    assert mean[0] == (100.0 + 101.0 + 100.0) / 3.0 and ratio[0] == mean[0] / sd[0]
    assert N.estimate(rows[1:], [0, 1, 2])['voxels'] == 0


def test_key_orders_like_the_values():
    v = np.array([-np.inf, -1.5, -0.0, 0.0, 5e-324, 1.0, np.inf])
    kk = N.key(v)
    assert (np.diff(kk.astype(object)) > 0).all()
    lo, hi, c = N.middles(np.array([0.0, -0.0, np.nan, np.nan]))
    assert c == 2 and np.signbit(lo) and not np.signbit(hi)
    assert N.middles(np.array([np.nan]))[2] == 0


# ---- configuration rules: all of them act in set_data, before a context exists or anything is uploaded
def small_image(n_b0, shape=(3, 3, 2)):
    sch = S.make_scheme(n_b0, ((1000.0, 8),), seed=1)
    return np.ones(shape + (sch.nS,), dtype=np.float32), sch


def test_key_defaults_to_off():
    import amico_amd
    ae = amico_amd.Evaluation()
    assert ae.get_config('doEstimateNoise') is False


@pytest.mark.parametrize('n_b0', [0, 1, 129])
def test_set_data_refuses_a_scheme_without_repeats(n_b0, monkeypatch):
    import amico_amd
    from amico_amd import prep
    monkeypatch.setattr(prep, 'SignalPreparation', lambda *a, **k: pytest.fail('set_data went on to the plan'))
    img, sch = small_image(n_b0)
    ae = amico_amd.Evaluation()
    ae.set_config('doEstimateNoise', True)
    with pytest.raises(RuntimeError, match='doEstimateNoise'):
        ae.set_data(img, sch)


def test_debias_without_snr_and_without_the_key_raises_as_before():
    import amico_amd
    img, sch = small_image(4)
    ae = amico_amd.Evaluation()
    ae.set_config('doDebiasSignal', True)
    with pytest.raises(RuntimeError) as e:
        ae.set_data(img, sch)
    assert str(e.value) == "Set noise variance for debiasing (eg. ae.set_config('RicianNoiseSigma', sigma))"


def test_bindings_are_declared():
    from amico_amd import _capi, noise
    hdr = open(os.path.join(ROOT, 'include', 'amico_amd.h')).read()
    declared = set(re.findall(r'\b(amx_[a-z0-9_]+)\s*\(', hdr))
    L = _capi.lib()
    for n in ['amx_noise_b0_rows_device', 'amx_noise_b0_rows_device_f32', 'amx_prep_noise_b0_device', 'amx_nanmedian_device']:
        assert n in declared and n in _capi.SYMBOLS and getattr(L, n).argtypes is not None, n
    assert 'gammaincinv' in hdr and 'sqrt(q / (k-1))' in hdr
    assert callable(_capi.Prep.noise_b0_device) and callable(_capi.noise_b0_rows_device) and callable(_capi.nanmedian_device)
    assert callable(noise.estimate_from_rows) and callable(noise.estimate_device)
