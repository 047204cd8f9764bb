"""The predicted signal on the CPU: the numpy restatement the GPU kernel is held to computes the intended quantity, and what a fit with
'doSavePredictedSignal' hands to the C ABI (the recorder of tests/test_capi_calls.py in place of the library: no GPU needed)."""
import numpy as np
import pytest
import torch

import predicted_np as P
from test_capi_calls import Ctx as _RecCtx, Recorder, labelled, make_lut, NA, NS

from amico_amd import _capi, models as M

N = 5


def test_restatement_is_a_times_x():
    """the sequential loop against A @ x in float64: 145 atoms in [0, 1], coefficients of unit scale -> |error| <= 145 eps * sum|a x|"""
    rng = np.random.default_rng(0)
    ndirs, nS, n_wm, n = 7, 13, 144, 200
    K = {'model': 'NODDI', 'wm': rng.uniform(0, 1, (n_wm, ndirs, nS)).astype(np.float32), 'iso': rng.uniform(0, 1, nS).astype(np.float32)}
    x = rng.uniform(0, 1, (n, n_wm + 1)) * (rng.uniform(size=(n, n_wm + 1)) < 0.1)
    idx = rng.integers(0, ndirs, n)
    idx[3] = -1
    got = P.predict_rows(K, x, idx)
    ok = idx >= 0
    A = P.dense_dictionaries(K, idx[ok])
    ref = np.einsum('nsj,nj->ns', A, x[ok])
    assert np.abs(got[ok] - ref).max() < 1e-13
    assert not got[3].any() and got.shape == (n, nS)
    # one dictionary for all voxels (SANDI's layout), a NaN coefficient
    Ks = {'model': 'SANDI', 'signal': np.asfortranarray(rng.uniform(0, 1, (6, 15)))}
    xs = rng.uniform(0, 1, (9, 15))
    xs[4, 7] = np.nan
    gs = P.predict_rows(Ks, xs)
    good = np.arange(9) != 4
    assert np.abs(gs[good] - xs[good] @ Ks['signal'].T).max() < 1e-13 and np.isnan(gs[4]).all()


class Ctx(_RecCtx):
    """the recorder's context with what a model's fit asks of one"""

    def sync(self, stream=None):
        pass

    def last_stats(self):
        return {'itercap_voxels': 0}


class Ev:
    def __init__(self, cfg, model):
        rng = np.random.default_rng(1)
        self.KERNELS, self.htable, self.nthreads, self.cfg = {'model': model.id}, np.zeros(4, np.int16), 1, cfg
        self._DIRs = None
        self._dev = {'y': torch.from_numpy(rng.random((N, NS))), 'dirs': torch.from_numpy(rng.random((N, 3)))}

    def get_config(self, key):
        return self.cfg.get(key)


CLASS = {'noddi': 'NODDI', 'freewater': 'FreeWater', 'sandi': 'SANDI', 'czb': 'CylinderZeppelinBall'}


@pytest.fixture
def ctxs():
    """the fake contexts of a test; emptied at its end, so that a handle that dies later never reaches a real library (Lut.close asks)"""
    made = []
    yield made
    for c in made:
        c._h = None


def _fit(monkeypatch, made, model, cfg):
    rec = Recorder()
    monkeypatch.setattr(_capi, '_lib', rec)
    ctx = Ctx()
    made.append(ctx)
    monkeypatch.setattr(M, 'get_context', lambda: ctx)
    monkeypatch.setattr(M, 'get_contexts', lambda: [ctx])
    m = getattr(M, CLASS[model])()
    if model == 'noddi':
        m.set(IC_VFs=np.array([0.5]), IC_ODs=np.array([0.1, 0.2, 0.3]))        # NA - 1 white-matter atoms
    if model == 'czb':
        m.set(Rs=np.array([1e-6, 2e-6]), d_perps=np.array([0.5e-3]), d_isos=np.array([2e-3]))
    lut = make_lut(ctx, model)
    monkeypatch.setattr(m, '_lut', lambda evaluation, builder, ctx=None: lut)
    ev = Ev(cfg, m)
    if model == 'noddi':
        ev.KERNELS['wm'] = np.zeros((NA - 1, 1, 1), np.float32)
    if model == 'czb':
        ev.KERNELS.update(wmr=np.zeros((2, 1, 1), np.float32), wmh=np.zeros((1, 1, 1), np.float32), iso=np.zeros((1, 1), np.float32))
    results = m.fit(ev)
    return rec, ctx, lut, ev, results


@pytest.mark.parametrize('model', list(CLASS))
def test_fit_with_the_key_adds_the_flag_and_one_predict_call(monkeypatch, ctxs, model):
    rec0, ctx0, lut0, ev0, res0 = _fit(monkeypatch, ctxs, model, {})
    plain = labelled(rec0.calls, ctx=ctx0._h, lut=lut0._h, y=ev0._dev['y'], dirs=ev0._dev['dirs'])
    assert len(plain) == 1 and 'y_est' not in res0 and 'predict' not in ev0._dev
    rec, ctx, lut, ev, res = _fit(monkeypatch, ctxs, model, {'doSavePredictedSignal': True})
    names = dict(ctx=ctx._h, lut=lut._h, y=ev._dev['y'], dirs=ev._dev['dirs'], x=ev._dev['predict'][1])
    calls = labelled(rec.calls, **names)
    # the unchanged fit call, AMX_F_DEBUG_X (16) added to its flags, behind the registration of the zeroed buffer
    flag = 'int:0, '
    assert plain[0].count(flag) == 1 + (model == 'freewater')           # (Free-Water: is_mouse, then the flags)
    head, tail = plain[0].rsplit(flag, 1)
    assert calls == ['amx_set_debug_x(ctx, x)', head + 'int:16, ' + tail]
    assert list(res) == list(res0) + ['y_est'] and len(rec.calls) == 2  # a key from the start, nothing made yet
    x = ev._dev['predict'][1]
    assert tuple(x.shape) == ((N, 3, NA) if model == 'noddi' else (N, NA)) and not x.any()
    # read: exactly one predict call, once
    ye = res['y_est']
    assert res['y_est'] is ye and ye.shape == (N, NS) and ye.dtype == np.float64
    more = labelled(rec.calls[2:], **names)
    stride, offset = (3 * NA, 2 * NA) if model == 'noddi' else (NA, 0)
    dirs = 'None' if model == 'sandi' else 'dirs'
    assert more == ['amx_predict_device(ctx, lut, x, int:%d, int:%d, %s, int:%d, unknown, None)' % (stride, offset, dirs, N)]


def test_key_with_an_assigned_y_or_several_devices_is_refused_before_any_upload(monkeypatch, ctxs):
    rec = Recorder()
    monkeypatch.setattr(_capi, '_lib', rec)
    ctx = Ctx()
    ctxs.append(ctx)
    monkeypatch.setattr(M, 'get_context', lambda: ctx)
    monkeypatch.setattr(M, 'get_contexts', lambda: [ctx])
    m = M.SANDI()
    ev = Ev({'doSavePredictedSignal': True}, m)
    ev._dev, ev.y, ev.DIRs = None, np.zeros((N, NS)), None
    with pytest.raises(NotImplementedError, match='doSavePredictedSignal'):
        m.fit(ev)
    ev2 = Ev({'doSavePredictedSignal': True}, m)
    monkeypatch.setattr(M, 'get_contexts', lambda: [ctx, ctx])
    with pytest.raises(NotImplementedError, match='several devices'):
        m.fit(ev2)
    assert rec.calls == []


def test_two_lazy_values_are_made_one_by_one():
    """Free-Water with both switches holds y_corrected and y_est: reading one makes that one only"""
    made = []
    r = M._LazyResults({'estimates': 0})
    r.set_lazy('y_corrected', lambda: made.append('c') or 1)
    r.set_lazy('y_est', lambda: made.append('e') or 2)
    assert list(r) == ['estimates', 'y_corrected', 'y_est'] and not made
    assert r['y_est'] == 2 and made == ['e'] and r['y_est'] == 2 and made == ['e']
    assert dict(r) == {'estimates': 0, 'y_corrected': 1, 'y_est': 2} and made == ['e', 'c']
