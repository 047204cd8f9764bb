"""The wild bootstrap without a GPU: the sign generator's statistics and its prefix / offset properties, the numpy restatement of the
replicate signal and of Welford's moments (tests/bootstrap_np.py, what tests/test_gpu_bootstrap.py holds the kernels to), the symbols,
and the refusals that are raised before anything touches a device."""
import os
import re

import numpy as np
import pytest

import bootstrap_np as B

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
N_VOX, SHAPES, SEEDS, REPLICATES = 1037, (6, 65, 99), (0, 7, 2 ** 63 + 5), 8


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('nS', SHAPES)
def test_signs_are_balanced_and_uncorrelated(nS, seed):
    """mean, replicate-to-replicate, adjacent-volume and adjacent-voxel correlations of N = 1037 * nS signs: each a mean of N (or
    nearly N) products of +-1, standard deviation 1 / sqrt(N) if the signs are independent -- held to 4 of them"""
    s = np.stack([B.signs(seed, b, 0, N_VOX, nS) for b in range(REPLICATES)])
    assert set(np.unique(s)) == {-1.0, 1.0}
    lim = 4.0 / np.sqrt(N_VOX * nS)
    flat = s.reshape(REPLICATES, -1)
    assert np.abs(flat.mean(axis=1)).max() < lim
    cross = flat @ flat.T / flat.shape[1]
    assert np.abs(cross - np.eye(REPLICATES)).max() < lim
    assert max(abs((r[:, 1:] * r[:, :-1]).mean()) for r in s) < lim
    assert max(abs((r[1:, :] * r[:-1, :]).mean()) for r in s) < lim


@pytest.mark.parametrize('seed', SEEDS)
def test_signs_depend_on_the_voxel_not_on_the_call(seed):
    """prefix: fewer voxels give the first rows; offset: first_voxel = k gives the rows from k on"""
    for nS in SHAPES:
        whole = B.signs(seed, 3, 0, 200, nS)
        assert np.array_equal(B.signs(seed, 3, 0, 50, nS), whole[:50])
        assert np.array_equal(B.signs(seed, 3, 100, 100, nS), whole[100:])
        assert np.array_equal(B.signs(seed, 3, 12345, 7, nS), B.signs(seed, 3, 12340, 12, nS)[5:])
        assert not np.array_equal(B.signs(seed, 4, 0, 200, nS), whole) and not np.array_equal(B.signs(seed + 1, 3, 0, 200, nS), whole)


def test_first_signs_are_the_recorded_ones():
    """the generator's constants, pinned by hand-computed values (python integers, no numpy)"""
    M = (1 << 64) - 1

    def sign(seed, b, ctr):
        z = (seed + (b + 1) * 0x9E3779B97F4A7C15 + ctr * 0xD1B54A32D192ED03) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        return -1.0 if z >> 63 else 1.0
    for seed, b, first, nS in ((0, 0, 0, 6), (2 ** 63 + 5, 97, 12345, 99), (7, 1, 2 ** 40, 65)):
        got = B.signs(seed, b, first, 3, nS)
        exp = np.array([[sign(seed, b, (first + i) * nS + j) for j in range(nS)] for i in range(3)])
        assert np.array_equal(got, exp)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_resample_clips_negatives_and_keeps_nan(dtype):
    rng = np.random.default_rng(1)
    n, nS = 40, 9
    ye = rng.uniform(0.1, 1.0, (n, nS))
    y = (ye + rng.normal(scale=0.05, size=ye.shape)).astype(dtype)
    y[3] = (ye[3] * 2.5).astype(dtype)                      # residual larger than the prediction: the mirrored sample is negative
    ye[5, 4] = np.nan
    y[7, 2] = np.nan
    yb = B.resample(y, ye, 11, 2)
    s = B.signs(11, 2, 0, n, nS)
    assert yb.dtype == dtype and yb.shape == y.shape
    assert np.isnan(yb[5, 4]) and np.isnan(yb[7, 2]) and np.isnan(yb).sum() == 2
    ok = ~np.isnan(yb)
    assert (yb[ok] >= 0).all()
    assert (yb[3][s[3] < 0] == 0).all() and (s[3] < 0).any()             # clipped
    keep = (s > 0) & ok
    assert np.array_equal(yb[keep], (ye + (y.astype(np.float64) - ye)).astype(dtype)[keep])      # s = +1: y again, to fp64 rounding
    flip = (s < 0) & ok & (np.arange(n)[:, None] != 3) & (np.nan_to_num(2 * ye - y) > 1e-3)      # (not clipped)
    assert np.allclose(yb[flip], (2 * ye - y)[flip], rtol=1e-6)
    # the first_voxel argument shifts the rows
    assert np.array_equal(B.resample(y[10:], ye[10:], 11, 2, first_voxel=10), yb[10:], equal_nan=True)


def test_welford_is_mean_and_std():
    rng = np.random.default_rng(2)
    for count in (2, 3, 5, 20):
        maps = [rng.uniform(0.0, 1.0, (57, 3)) for _ in range(count)]
        mean, std = B.welford(maps)
        assert np.abs(mean - np.mean(maps, axis=0)).max() < 1e-12
        assert np.abs(std - np.std(maps, axis=0, ddof=1)).max() < 1e-12
    maps[1][4, 2] = np.nan
    mean, std = B.welford(maps)
    assert np.isnan(mean[4, 2]) and np.isnan(std[4, 2]) and np.isnan(mean).sum() == 1 and np.isnan(std).sum() == 1


def test_bootstrap_symbols_declared_and_bound():
    from amico_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'amico_amd.h')).read()
    declared = set(re.findall(r'\b(amx_[a-z0-9_]+)\s*\(', hdr))
    names = ['amx_bootstrap_resample_device', 'amx_bootstrap_resample_device_f32', 'amx_bootstrap_accumulate_device',
             'amx_bootstrap_std_device']
    L = _capi.lib()
    for n in names:
        assert n in declared and n in _capi.SYMBOLS and getattr(L, n).argtypes is not None, n
    assert '0x9E3779B97F4A7C15' in hdr and '0xD1B54A32D192ED03' in hdr and 'core.py:452' in hdr
    for fn in ('bootstrap_resample_device', 'bootstrap_accumulate_device', 'bootstrap_std_device'):
        assert callable(getattr(_capi, fn))


@pytest.mark.parametrize('bad', [1, -3, 10001, 2.5, '4', True, [4]])
def test_bad_sample_counts_are_value_errors(bad):
    from amico_amd import bootstrap
    with pytest.raises(ValueError, match='bootstrap_samples'):
        bootstrap.check_samples(bad)
    with pytest.raises(ValueError, match='bootstrap_samples'):          # before the context or any tensor is looked at
        bootstrap.wild_bootstrap(None, None, None, None, None, 0.0, 0.0, (), None, bad)


def test_sample_counts_and_seeds_that_pass():
    from amico_amd import bootstrap
    assert bootstrap.check_samples(2) == 2 and bootstrap.check_samples(np.int64(10000)) == 10000
    assert bootstrap.check_seed(2 ** 64 - 1) == 2 ** 64 - 1 and bootstrap.check_seed(np.uint64(5)) == 5
    for bad in (-1, 2 ** 64, 0.5, None):
        with pytest.raises(ValueError, match='bootstrap_seed'):
            bootstrap.check_seed(bad)


class _Ev:
    """the fields a model's fit reads, without data: enough to reach the refusals"""

    def __init__(self, cfg, model_id):
        self.cfg, self.nthreads, self.htable, self._dev = cfg, 1, None, None
        self.y, self.DIRs, self.KERNELS = np.zeros((4, 6)), np.zeros((4, 3)), {'model': model_id}

    def get_config(self, key):
        return self.cfg.get(key)


def _no_gpu(monkeypatch):
    """a context stand-in: the refusals come before anything would be asked of it"""
    from amico_amd import models as M
    ctx = object()
    monkeypatch.setattr(M, 'get_contexts', lambda: [ctx])
    monkeypatch.setattr(M, 'get_context', lambda: ctx)
    return M


def test_config_reads_the_two_keys():
    from amico_amd import bootstrap
    assert bootstrap.config(_Ev({}, 'NODDI')) is None
    assert bootstrap.config(_Ev({'bootstrap_samples': None, 'bootstrap_seed': 3}, 'NODDI')) is None
    assert bootstrap.config(_Ev({'bootstrap_samples': 0}, 'NODDI')) is None
    assert bootstrap.config(_Ev({'bootstrap_samples': 100}, 'NODDI')) == (100, 0)
    assert bootstrap.config(_Ev({'bootstrap_samples': 4, 'bootstrap_seed': 7}, 'NODDI')) == (4, 7)
    with pytest.raises(ValueError, match='bootstrap_samples'):
        bootstrap.config(_Ev({'bootstrap_samples': 1}, 'NODDI'))
    with pytest.raises(ValueError, match='bootstrap_seed'):
        bootstrap.config(_Ev({'bootstrap_samples': 4, 'bootstrap_seed': -1}, 'NODDI'))


def test_model_fit_refuses_before_anything_is_uploaded(monkeypatch):
    M = _no_gpu(monkeypatch)
    uploads = []
    from amico_amd import _capi
    monkeypatch.setattr(_capi, 'upload_sandi', lambda *a, **k: uploads.append(a))
    sandi = M.SANDI()
    with pytest.raises(ValueError, match='bootstrap_samples'):
        sandi.fit(_Ev({'bootstrap_samples': 1}, 'SANDI'))
    # an assigned evaluation.y (no device-resident signals)
    with pytest.raises(NotImplementedError, match='bootstrap_samples'):
        sandi.fit(_Ev({'bootstrap_samples': 4}, 'SANDI'))
    # SANDI, with device-resident signals
    ev = _Ev({'bootstrap_samples': 4}, 'SANDI')
    ev._dev = {'y': np.zeros((4, 6), np.float32)}
    with pytest.raises(NotImplementedError, match='SANDI.*residuals mean nothing'):
        sandi.fit(ev)
    # several devices
    monkeypatch.setattr(M, 'get_contexts', lambda: [object(), object()])
    with pytest.raises(NotImplementedError, match='several devices'):
        sandi.fit(ev)
    assert not uploads


def test_wild_bootstrap_refuses_sandi():
    from amico_amd import _capi, bootstrap
    with pytest.raises(NotImplementedError, match='residuals mean nothing'):
        bootstrap.wild_bootstrap(None, _capi.FIT['sandi'], None, None, None, 0.0, 5e-3, (), None, 4)


def test_evaluation_refuses_before_anything_is_uploaded(monkeypatch):
    """Evaluation.fit says the same three things before it makes a device buffer"""
    import amico_amd
    from amico_amd import core
    ae = amico_amd.Evaluation()
    ae._img32 = np.zeros((2, 2, 2, 6), np.float32)          # "data loaded" for fit()'s own order of checks
    ae.model = amico_amd.SANDI()
    ae.KERNELS = {'model': 'SANDI'}
    ae.set_config('bootstrap_samples', 10001)
    with pytest.raises(ValueError, match='bootstrap_samples'):
        ae.fit()
    ae.set_config('bootstrap_samples', 4)
    with pytest.raises(NotImplementedError, match='residuals mean nothing'):
        ae.fit()
    ae.model = amico_amd.NODDI()
    ae.KERNELS = {'model': 'NODDI'}
    monkeypatch.setattr(core._models, 'get_contexts', lambda: [object(), object()])
    with pytest.raises(NotImplementedError, match='several devices'):
        ae.fit()
