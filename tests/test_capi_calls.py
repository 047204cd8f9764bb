"""What amico_amd._capi and amico_amd.pipeline hand to the C ABI, call by call, on the CPU: the library is replaced by a recorder, so no
library and no GPU are needed.  Every pointer argument is recorded by the ROLE of the buffer it points to (y, dirs, out[k], ...), every
scalar by type and value.  The expected records at the end of this file were written by `records()` of this file run on the commit
BEFORE the bindings of the four fits were folded into one table-driven layer (the eight hand-written wrappers, the pipelines calling
ctypes symbols themselves); they are not edited: the layer has to reproduce them call for call."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from amico_amd import _capi

N, NS, NA, NISO = 5, 7, 4, 2            # voxels, volumes, atoms, isotropic atoms: small and all different
MODELS = ('noddi', 'freewater', 'sandi', 'czb')


class Recorder:
    """stands in for the loaded library: every attribute is a function that notes (symbol, args) and returns its status (0)"""

    def __init__(self):
        self.calls, self.status = [], {}

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.status.get(name, 0)
        return fn


class Ctx:
    def __init__(self):
        self._h = C.c_void_p(0xC0)

    def check(self, rc):
        if rc != 0:
            raise RuntimeError('status %d' % rc)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_capi, '_lib', r)
    r.ctx = Ctx()
    yield r
    r.ctx._h = None             # (handles that die after the recorder is gone must not reach a real library: close() asks the context)


def _address(a):
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, C._Pointer):
        return C.cast(a, C.c_void_p).value
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def labelled(calls, **buffers):
    """the calls as strings; `buffers`: role -> array / tensor / handle (None entries are skipped; a tuple gives role[k]).  The *_destroy
    calls are left out: when a handle's owner is collected is not what is recorded here"""
    roles = {}
    for name, b in buffers.items():
        for k, e in enumerate(b) if isinstance(b, (tuple, list)) else [(None, b)]:
            if e is not None:
                roles[_address(e)] = name if k is None else '%s[%d]' % (name, k)

    def one(a):
        if a is None:
            return 'None'
        if isinstance(a, (C.c_void_p, C._Pointer)):
            return 'None' if _address(a) is None else roles.get(_address(a), 'unknown')
        if type(a) is int and a in roles:
            return roles[a]
        return '%s:%r' % (type(a).__name__, a) if type(a) in (int, float, bool, str) else 'unknown'
    return ['%s(%s)' % (sym, ', '.join(one(a) for a in args)) for sym, args in calls if not sym.endswith('_destroy')]


def shapes(res):
    return [None if a is None else '%s%s' % (str(a.dtype).replace('torch.', ''), tuple(a.shape)) for a in res]


def make_lut(ctx, model):
    lut = _capi.Lut(ctx, C.c_void_p(0x107), model, NS, NA, {'noddi': 3, 'sandi': 6, 'czb': 3}.get(model))
    if model == 'freewater':
        lut.n_iso = NISO
    return lut


def fit_args(model, opts):
    """(extra positional arguments behind lambda2, keywords) of the public wrapper: every optional output on or off"""
    extras = {'noddi': (3,), 'freewater': (opts,)}.get(model, ())      # (Free-Water: Human without, Mouse with the optional outputs)
    kw = dict(rmse=opts, nrmse=opts)
    if model == 'noddi':
        kw['mod'] = opts
    if model == 'freewater':
        kw['corrected'] = opts
    return extras, kw


def inputs(model, form, dtype):
    rng = np.random.default_rng(3)
    y = rng.random((N, NS)).astype(dtype)
    dirs = None if model == 'sandi' else rng.random((N, 3))
    if form == 'device':
        y, dirs = torch.from_numpy(y), None if dirs is None else torch.from_numpy(dirs)
    return y, dirs


def run_fit(rec, model, form, dtype, opts, **more):
    y, dirs = inputs(model, form, dtype)
    lut = make_lut(rec.ctx, model)
    extras, kw = fit_args(model, opts)
    kw.update(more)
    fn = getattr(_capi, model + ('_fit_device' if form == 'device' else '_fit'))
    pos = (rec.ctx, lut, y) + (() if dirs is None else (dirs,)) + (0.5, 0.001) + extras
    try:
        res, err = fn(*pos, **kw), None
    except RuntimeError as e:
        res, err = (), str(e)
    n_out = 3 + (model in ('noddi', 'freewater'))
    named = dict(out=res[:n_out])
    rest = list(res[n_out:])
    if more.get('return_x'):
        named['x_debug'] = rest.pop(0)
        assert not named['x_debug'].any()                 # the debug buffer is handed over zeroed
    if more.get('iso') and rest:
        named['x_iso'] = rest.pop(0)
    if more.get('out') is not None:
        assert all(a is b for a, b in zip(res, more['out']))
    return {'calls': labelled(rec.calls, ctx=rec.ctx._h, lut=lut._h, y=y, dirs=dirs, **named), 'returns': shapes(res), 'error': err}


def fit_cases():
    for model, form, dtype, opts in itertools.product(MODELS, ('host', 'device'), ('float64', 'float32'), (False, True)):
        yield '%s %s %s %s' % (model, form, dtype, 'all' if opts else 'none'), (model, form, dtype, opts), {}
    for model in MODELS:
        yield '%s device float64 return_x' % model, (model, 'device', 'float64', False), dict(return_x=True)
    yield 'freewater device float32 iso', ('freewater', 'device', 'float32', False), dict(iso=True)
    yield 'freewater device float64 iso return_x all', ('freewater', 'device', 'float64', True), dict(iso=True, return_x=True)


# ---- the two pipelines: built on the recorder (plan, tensor helper and dictionary are handles the recorder never fills), then enqueue()
def make_pipeline(rec, monkeypatch, model, raw_dtype, replace, debias, fused, corrected):
    from amico_amd import pipeline, synthetic
    monkeypatch.setattr(pipeline, 'get_context', lambda: rec.ctx)
    sch = synthetic.make_scheme(n_b0=1, shells=((1000.0, NS - 1),))
    img = np.ones((2, 2, 2, NS), dtype=np.int16 if raw_dtype else np.float32)
    mask = np.ones((2, 2, 2), dtype=np.uint8)
    mask[0, 0, 0] = mask[1, 0, 1] = 0
    ht = np.zeros(181 * 181, dtype=np.int16)
    kw = dict(device=torch.device('cpu'), fused=fused, debias_snr=20.0 if debias else None, replace_bad_voxels=0.25 if replace else None,
              raw_dtype=np.int16 if raw_dtype else None)
    if model == 'noddi':
        K = {'wm': np.ones((NA - 1, 3, NS), np.float32), 'iso': np.ones(NS, np.float32), 'norms': np.ones((NS - 1, NA - 1)),
             'icvf': np.ones(NA - 1, np.float32), 'kappa': np.ones(NA - 1, np.float32)}
        pl = pipeline.NoddiVolumePipeline(sch, img, mask, K, ht, **kw)
    else:
        K = {'D': np.ones((NA - NISO, 3, NS), np.float32), 'CSF': np.ones((NISO, NS), np.float32)}
        pl = pipeline.FreeWaterVolumePipeline(sch, img, mask, K, ht, corrected=corrected, is_mouse=True, **kw)
    pl.prep._plan._h, pl.tensor._dti._h, pl.lut._h = C.c_void_p(0x9A), C.c_void_p(0xD7), C.c_void_p(0x107)
    return pl, torch.from_numpy(img.reshape(-1).copy())


def run_pipeline(rec, monkeypatch, *case):
    pl, d_img = make_pipeline(rec, monkeypatch, *case)
    del rec.calls[:]
    pl.enqueue(d_img, stream=0x57)
    return labelled(rec.calls, ctx=rec.ctx._h, plan=pl.prep._plan._h, dti=pl.tensor._dti._h, lut=pl.lut._h, d_img=d_img, img=pl.img,
                    y=pl.y, mean_b0=pl.mean_b0, dirs=pl.dirs, est=pl.est, maps=pl.maps, dirs_vol=pl.dirs_vol,
                    x_iso=getattr(pl, 'x_iso', None), corrected=getattr(pl, 'corrected', None), stream=C.c_void_p(0x57))


def pipeline_cases():
    for model in ('noddi', 'freewater'):
        for sw in itertools.product((False, True), repeat=5 if model == 'freewater' else 4):
            names = [n for n, on in zip(('raw_dtype', 'replace', 'debias', 'fused', 'corrected'), sw) if on]
            yield '%s pipeline %s' % (model, ' '.join(names) or 'plain'), (model,) + sw + (False,) * (5 - len(sw))


def records(rec, monkeypatch):
    """every record of this file, by name"""
    out = {}
    for name, case, more in fit_cases():
        del rec.calls[:]
        out[name] = run_fit(rec, *case, **more)
    rec.status = {'amx_freewater_fit_device_f32': -2}
    del rec.calls[:]
    out['freewater device float32 iso, the fit fails'] = run_fit(rec, 'freewater', 'device', 'float32', False, iso=True)
    rec.status = {}
    for model in MODELS:                     # out= given: the caller's arrays are the ones written and returned
        del rec.calls[:]
        w = {'noddi': 3, 'freewater': 4, 'sandi': 6, 'czb': 3}[model]
        o = (np.zeros((N, w)), np.zeros(N), np.zeros(N)) + {'noddi': (np.zeros((N, 2)),), 'freewater': (np.zeros((N, NS)),)}.get(model, ())
        out['%s host float64 all out=' % model] = run_fit(rec, model, 'host', 'float64', True, out=o)
    for name, case in pipeline_cases():
        out[name] = run_pipeline(rec, monkeypatch, *case)
    return out


def generate(monkeypatch):
    """records() on a recorder of its own: what wrote EXPECTED below"""
    r = Recorder()
    monkeypatch.setattr(_capi, '_lib', r)
    r.ctx = Ctx()
    out = records(r, monkeypatch)
    r.ctx._h = None
    return out


def test_every_call_is_the_one_recorded_before_the_refactor(rec, monkeypatch):
    got = records(rec, monkeypatch)
    assert sorted(got) == sorted(EXPECTED)
    for name in EXPECTED:
        assert got[name] == EXPECTED[name], name


def test_fw_iso_is_unregistered_when_the_fit_fails(rec):
    rec.status = {'amx_freewater_fit_device_f32': -2}
    r = run_fit(rec, 'freewater', 'device', 'float32', False, iso=True)
    assert r['error'] == 'status -2'
    assert [c.split('(')[0] for c in r['calls']] == ['amx_set_fw_iso', 'amx_freewater_fit_device_f32', 'amx_set_fw_iso']
    assert r['calls'][-1] == 'amx_set_fw_iso(ctx, None)' and r['calls'][0].startswith('amx_set_fw_iso(ctx, ') and r['calls'][0] != r['calls'][-1]


OUT_FAULTS = [('dtype', lambda: np.zeros((N, 3), dtype=np.float32)), ('shape', lambda: np.zeros((N + 1, 3))),
              ('contiguity', lambda: np.zeros((3, N)).T), ('writable', lambda: np.zeros((N, 3)))]


@pytest.mark.parametrize('fault', [f[0] for f in OUT_FAULTS])
def test_out_arrays_are_checked(rec, fault):
    y, dirs = inputs('czb', 'host', 'float64')
    est = dict(OUT_FAULTS)[fault]()
    if fault == 'writable':
        est.setflags(write=False)
    with pytest.raises(ValueError) as e:
        _capi.czb_fit(rec.ctx, make_lut(rec.ctx, 'czb'), y, dirs, 0.0, 4.0, out=(est, None, None))
    assert str(e.value) == 'out[0] must be a writable C-contiguous float64 array of shape ((5, 3),)'
    assert labelled(rec.calls) == []
    with pytest.raises(ValueError) as e:
        _capi.sandi_fit(rec.ctx, make_lut(rec.ctx, 'sandi'), y, 0.0, 4.0, rmse=True, out=(None, np.zeros(N + 1), None))
    assert str(e.value) == 'out[1] must be a writable C-contiguous float64 array of shape ((5,),)'


def test_error_texts(rec):
    """every ValueError of the fit wrappers, as whole strings"""
    ctx = rec.ctx
    y, dirs = inputs('noddi', 'host', 'float64')
    ty, td = torch.from_numpy(y), torch.from_numpy(dirs)

    def text(fn, *a, **k):
        with pytest.raises(ValueError) as e:
            fn(*a, **k)
        return str(e.value)
    n_maps = 'the dictionary writes 3 maps per voxel, the model expects 4 (isExvivo changed?)'
    assert text(_capi.noddi_fit, ctx, make_lut(ctx, 'noddi'), y, dirs, 0.5, 0.001, 4) == n_maps
    assert text(_capi.noddi_fit_device, ctx, make_lut(ctx, 'noddi'), ty, td, 0.5, 0.001, 4) == n_maps
    bad_y = 'y must be [n_vox, 7] float64 (or float32)'
    bad_dirs = 'DIRs must be [n_vox, 3]'
    dev_y = 'y must be a contiguous float64 (or float32) device tensor [n_vox, 7] (the dictionary was built for 7 volumes per voxel)'
    dev_dirs = 'DIRs must be a contiguous float64 device tensor [n_vox, 3] on the device of y'
    for model in MODELS:
        lut = make_lut(ctx, model)
        extras, _ = fit_args(model, False)
        host, dev = getattr(_capi, model + '_fit'), getattr(_capi, model + '_fit_device')
        d, t = ((), ()) if model == 'sandi' else ((dirs,), (td,))
        assert text(host, ctx, lut, y[:, :6], *d, 0.5, 0.001, *extras) == bad_y
        assert text(host, ctx, lut, y[0], *d, 0.5, 0.001, *extras) == bad_y
        assert text(dev, ctx, lut, ty[:, :6].contiguous(), *t, 0.5, 0.001, *extras) == dev_y
        assert text(dev, ctx, lut, ty.T.contiguous().T, *t, 0.5, 0.001, *extras) == dev_y
        assert text(dev, ctx, lut, ty.to(torch.float16), *t, 0.5, 0.001, *extras) == dev_y
        if model != 'sandi':
            assert text(host, ctx, lut, y, dirs[:4], 0.5, 0.001, *extras) == bad_dirs
            assert text(dev, ctx, lut, ty, td[:4], 0.5, 0.001, *extras) == dev_dirs
            assert text(dev, ctx, lut, ty, td.to(torch.float32), 0.5, 0.001, *extras) == dev_dirs
    lut = make_lut(ctx, 'freewater')
    x_iso = 'x_iso must be a contiguous float64 device tensor [n_vox, 2] on the device of y'
    assert text(_capi.freewater_corrected_device, ctx, lut, ty, torch.zeros((N, 3), dtype=torch.float64)) == x_iso
    assert text(_capi.freewater_corrected_device, ctx, lut, ty, torch.zeros((N, NISO), dtype=torch.float32)) == x_iso
    assert labelled(rec.calls) == []


def test_tensors_handed_to_the_device_fit_are_checked(rec):
    """_fit_device(into=, iso=<tensor>): what a pipeline hands in is checked like out= of the host form -- dtype, shape, contiguity"""
    y, dirs = inputs('freewater', 'device', 'float32')
    lut = make_lut(rec.ctx, 'freewater')

    def fit(**k):
        return _capi._fit_device(_capi.FIT['freewater'], rec.ctx, lut, y, dirs, 0.0, 0.001, (1,), {}, None, False, k.pop('iso', False), **k)
    f64 = torch.float64
    for bad in (torch.zeros((N, 4), dtype=torch.float32), torch.zeros((N, 2), dtype=f64), torch.zeros((4, N), dtype=f64).T):
        with pytest.raises(ValueError) as e:
            fit(into=bad)
        assert str(e.value) == 'into must be a contiguous float64 device tensor of shape ((5, 4),) on the device of y'
    for bad in (torch.zeros((N, NISO), dtype=torch.float32), torch.zeros((N, 3), dtype=f64), torch.zeros((NISO, N), dtype=f64).T):
        with pytest.raises(ValueError) as e:
            fit(iso=bad)
        assert str(e.value) == 'iso must be a contiguous float64 device tensor of shape ((5, 2),) on the device of y'
    assert labelled(rec.calls) == []
    est, xi = torch.zeros((N, 4), dtype=f64), torch.zeros((N, NISO), dtype=f64)
    res = fit(into=est, iso=xi)
    assert res[0] is est and res[-1] is xi and len(res) == 5
    assert labelled(rec.calls, ctx=rec.ctx._h, lut=lut._h, y=y, dirs=dirs, est=est, xi=xi) == [
        'amx_set_fw_iso(ctx, xi)',
        'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:5, float:0.0, float:0.001, int:1, int:32, est, None, None, None, None)',
        'amx_set_fw_iso(ctx, None)']


# ---- recorded on the commit before the refactor (see the docstring of this file)
EXPECTED = {'noddi host float64 none': {'calls': ['amx_noddi_fit(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, out[0], None, None, None)'],
                             'returns': ['float64(5, 3)', None, None, None],
                             'error': None},
 'noddi host float64 all': {'calls': ['amx_noddi_fit(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:7, out[0], out[1], out[2], out[3])'],
                            'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)', 'float64(5, 2)'],
                            'error': None},
 'noddi host float32 none': {'calls': ['amx_noddi_fit_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, out[0], None, None, None)'],
                             'returns': ['float64(5, 3)', None, None, None],
                             'error': None},
 'noddi host float32 all': {'calls': ['amx_noddi_fit_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:7, out[0], out[1], out[2], out[3])'],
                            'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)', 'float64(5, 2)'],
                            'error': None},
 'noddi device float64 none': {'calls': ['amx_noddi_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, out[0], None, None, None, None)'],
                               'returns': ['float64(5, 3)', None, None, None],
                               'error': None},
 'noddi device float64 all': {'calls': ['amx_noddi_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:7, out[0], out[1], out[2], out[3], None)'],
                              'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)', 'float64(5, 2)'],
                              'error': None},
 'noddi device float32 none': {'calls': ['amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, out[0], None, None, None, None)'],
                               'returns': ['float64(5, 3)', None, None, None],
                               'error': None},
 'noddi device float32 all': {'calls': ['amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:7, out[0], out[1], out[2], out[3], '
                                        'None)'],
                              'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)', 'float64(5, 2)'],
                              'error': None},
 'freewater host float64 none': {'calls': ['amx_freewater_fit(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, int:0, out[0], None, None, None)'],
                                 'returns': ['float64(5, 2)', None, None, None],
                                 'error': None},
 'freewater host float64 all': {'calls': ['amx_freewater_fit(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:1, int:11, out[0], out[1], out[2], out[3])'],
                                'returns': ['float64(5, 4)', 'float64(5,)', 'float64(5,)', 'float64(5, 7)'],
                                'error': None},
 'freewater host float32 none': {'calls': ['amx_freewater_fit_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, int:0, out[0], None, None, None)'],
                                 'returns': ['float64(5, 2)', None, None, None],
                                 'error': None},
 'freewater host float32 all': {'calls': ['amx_freewater_fit_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:1, int:11, out[0], out[1], out[2], '
                                          'out[3])'],
                                'returns': ['float64(5, 4)', 'float64(5,)', 'float64(5,)', 'float64(5, 7)'],
                                'error': None},
 'freewater device float64 none': {'calls': ['amx_freewater_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, int:0, out[0], None, None, '
                                             'None, None)'],
                                   'returns': ['float64(5, 2)', None, None, None],
                                   'error': None},
 'freewater device float64 all': {'calls': ['amx_freewater_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:1, int:11, out[0], out[1], out[2], '
                                            'out[3], None)'],
                                  'returns': ['float64(5, 4)', 'float64(5,)', 'float64(5,)', 'float64(5, 7)'],
                                  'error': None},
 'freewater device float32 none': {'calls': ['amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, int:0, out[0], None, None, '
                                             'None, None)'],
                                   'returns': ['float64(5, 2)', None, None, None],
                                   'error': None},
 'freewater device float32 all': {'calls': ['amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:1, int:11, out[0], out[1], '
                                            'out[2], out[3], None)'],
                                  'returns': ['float64(5, 4)', 'float64(5,)', 'float64(5,)', 'float64(5, 7)'],
                                  'error': None},
 'sandi host float64 none': {'calls': ['amx_sandi_fit(ctx, lut, y, int:5, float:0.5, float:0.001, int:0, out[0], None, None)'],
                             'returns': ['float64(5, 6)', None, None],
                             'error': None},
 'sandi host float64 all': {'calls': ['amx_sandi_fit(ctx, lut, y, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2])'],
                            'returns': ['float64(5, 6)', 'float64(5,)', 'float64(5,)'],
                            'error': None},
 'sandi host float32 none': {'calls': ['amx_sandi_fit_f32(ctx, lut, y, int:5, float:0.5, float:0.001, int:0, out[0], None, None)'],
                             'returns': ['float64(5, 6)', None, None],
                             'error': None},
 'sandi host float32 all': {'calls': ['amx_sandi_fit_f32(ctx, lut, y, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2])'],
                            'returns': ['float64(5, 6)', 'float64(5,)', 'float64(5,)'],
                            'error': None},
 'sandi device float64 none': {'calls': ['amx_sandi_fit_device(ctx, lut, y, int:5, float:0.5, float:0.001, int:0, out[0], None, None, None)'],
                               'returns': ['float64(5, 6)', None, None],
                               'error': None},
 'sandi device float64 all': {'calls': ['amx_sandi_fit_device(ctx, lut, y, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2], None)'],
                              'returns': ['float64(5, 6)', 'float64(5,)', 'float64(5,)'],
                              'error': None},
 'sandi device float32 none': {'calls': ['amx_sandi_fit_device_f32(ctx, lut, y, int:5, float:0.5, float:0.001, int:0, out[0], None, None, None)'],
                               'returns': ['float64(5, 6)', None, None],
                               'error': None},
 'sandi device float32 all': {'calls': ['amx_sandi_fit_device_f32(ctx, lut, y, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2], None)'],
                              'returns': ['float64(5, 6)', 'float64(5,)', 'float64(5,)'],
                              'error': None},
 'czb host float64 none': {'calls': ['amx_czb_fit(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, out[0], None, None)'],
                           'returns': ['float64(5, 3)', None, None],
                           'error': None},
 'czb host float64 all': {'calls': ['amx_czb_fit(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2])'],
                          'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)'],
                          'error': None},
 'czb host float32 none': {'calls': ['amx_czb_fit_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, out[0], None, None)'],
                           'returns': ['float64(5, 3)', None, None],
                           'error': None},
 'czb host float32 all': {'calls': ['amx_czb_fit_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2])'],
                          'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)'],
                          'error': None},
 'czb device float64 none': {'calls': ['amx_czb_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, out[0], None, None, None)'],
                             'returns': ['float64(5, 3)', None, None],
                             'error': None},
 'czb device float64 all': {'calls': ['amx_czb_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2], None)'],
                            'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)'],
                            'error': None},
 'czb device float32 none': {'calls': ['amx_czb_fit_device_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, out[0], None, None, None)'],
                             'returns': ['float64(5, 3)', None, None],
                             'error': None},
 'czb device float32 all': {'calls': ['amx_czb_fit_device_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2], None)'],
                            'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)'],
                            'error': None},
 'noddi device float64 return_x': {'calls': ['amx_set_debug_x(ctx, x_debug)',
                                             'amx_noddi_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:16, out[0], None, None, None, None)'],
                                   'returns': ['float64(5, 3)', None, None, None, 'float64(5, 3, 4)'],
                                   'error': None},
 'freewater device float64 return_x': {'calls': ['amx_set_debug_x(ctx, x_debug)',
                                                 'amx_freewater_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, int:16, out[0], None, '
                                                 'None, None, None)'],
                                       'returns': ['float64(5, 2)', None, None, None, 'float64(5, 4)'],
                                       'error': None},
 'sandi device float64 return_x': {'calls': ['amx_set_debug_x(ctx, x_debug)',
                                             'amx_sandi_fit_device(ctx, lut, y, int:5, float:0.5, float:0.001, int:16, out[0], None, None, None)'],
                                   'returns': ['float64(5, 6)', None, None, 'float64(5, 4)'],
                                   'error': None},
 'czb device float64 return_x': {'calls': ['amx_set_debug_x(ctx, x_debug)',
                                           'amx_czb_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:16, out[0], None, None, None)'],
                                 'returns': ['float64(5, 3)', None, None, 'float64(5, 4)'],
                                 'error': None},
 'freewater device float32 iso': {'calls': ['amx_set_fw_iso(ctx, x_iso)',
                                            'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, int:32, out[0], None, None, '
                                            'None, None)',
                                            'amx_set_fw_iso(ctx, None)'],
                                  'returns': ['float64(5, 2)', None, None, None, 'float64(5, 2)'],
                                  'error': None},
 'freewater device float64 iso return_x all': {'calls': ['amx_set_debug_x(ctx, x_debug)',
                                                         'amx_set_fw_iso(ctx, x_iso)',
                                                         'amx_freewater_fit_device(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:1, int:59, out[0], '
                                                         'out[1], out[2], out[3], None)',
                                                         'amx_set_fw_iso(ctx, None)'],
                                               'returns': ['float64(5, 4)', 'float64(5,)', 'float64(5,)', 'float64(5, 7)', 'float64(5, 4)', 'float64(5, 2)'],
                                               'error': None},
 'freewater device float32 iso, the fit fails': {'calls': ['amx_set_fw_iso(ctx, unknown)',
                                                           'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:0, int:32, '
                                                           'unknown, None, None, None, None)',
                                                           'amx_set_fw_iso(ctx, None)'],
                                                 'returns': [],
                                                 'error': 'status -2'},
 'noddi host float64 all out=': {'calls': ['amx_noddi_fit(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:7, out[0], out[1], out[2], out[3])'],
                                 'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)', 'float64(5, 2)'],
                                 'error': None},
 'freewater host float64 all out=': {'calls': ['amx_freewater_fit(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:1, int:11, out[0], out[1], out[2], '
                                               'out[3])'],
                                     'returns': ['float64(5, 4)', 'float64(5,)', 'float64(5,)', 'float64(5, 7)'],
                                     'error': None},
 'sandi host float64 all out=': {'calls': ['amx_sandi_fit(ctx, lut, y, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2])'],
                                 'returns': ['float64(5, 6)', 'float64(5,)', 'float64(5,)'],
                                 'error': None},
 'czb host float64 all out=': {'calls': ['amx_czb_fit(ctx, lut, y, dirs, int:5, float:0.5, float:0.001, int:3, out[0], out[1], out[2])'],
                               'returns': ['float64(5, 3)', 'float64(5,)', 'float64(5,)'],
                               'error': None},
 'noddi pipeline plain': ['amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                          'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                          'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                          'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                          'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline fused': ['amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                          'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                          'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                          'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline debias': ['amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                           'amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                           'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                           'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                           'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                           'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline debias fused': ['amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                 'amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                 'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                 'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                 'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline replace': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                            'amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                            'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                            'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                            'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                            'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                            'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline replace fused': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                  'amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                  'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                  'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                  'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                  'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline replace debias': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                   'amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                   'amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                                   'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                   'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                   'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                   'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                   'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline replace debias fused': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                         'amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                         'amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                         'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                         'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                         'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                         'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline raw_dtype': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                              'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                              'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                              'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                              'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                              'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline raw_dtype fused': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                    'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                    'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                    'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                    'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline raw_dtype debias': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                     'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                     'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                     'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                     'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                     'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                     'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline raw_dtype debias fused': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                           'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                           'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                           'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                           'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                           'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline raw_dtype replace': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, stream)',
                                      'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                      'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                      'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                      'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                      'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                      'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline raw_dtype replace fused': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, stream)',
                                            'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                            'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                            'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                            'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                            'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline raw_dtype replace debias': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, stream)',
                                             'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                             'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                             'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                             'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                             'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, stream)',
                                             'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                             'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'noddi pipeline raw_dtype replace debias fused': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, stream)',
                                                   'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                                   'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                                   'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                   'amx_noddi_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.5, float:0.001, int:0, est, None, None, None, '
                                                   'stream)',
                                                   'amx_prep_scatter_device(ctx, plan, est, int:3, maps, stream)',
                                                   'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline plain': ['amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                              'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                              'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, stream)',
                              'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                              'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline corrected': ['amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                                  'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                  'amx_set_fw_iso(ctx, x_iso)',
                                  'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, None, None, '
                                  'stream)',
                                  'amx_set_fw_iso(ctx, None)',
                                  'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                  'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                  'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline fused': ['amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                              'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, stream)',
                              'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                              'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline fused corrected': ['amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                        'amx_set_fw_iso(ctx, x_iso)',
                                        'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, None, None, '
                                        'stream)',
                                        'amx_set_fw_iso(ctx, None)',
                                        'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                        'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                        'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline debias': ['amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                               'amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                               'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                               'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, stream)',
                               'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                               'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline debias corrected': ['amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                         'amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                                         'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                         'amx_set_fw_iso(ctx, x_iso)',
                                         'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, None, None, '
                                         'stream)',
                                         'amx_set_fw_iso(ctx, None)',
                                         'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                         'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                         'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline debias fused': ['amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                     'amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                     'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, '
                                     'stream)',
                                     'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                     'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline debias fused corrected': ['amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                               'amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                               'amx_set_fw_iso(ctx, x_iso)',
                                               'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, None, '
                                               'None, stream)',
                                               'amx_set_fw_iso(ctx, None)',
                                               'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                               'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                               'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline replace': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                'amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                                'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, stream)',
                                'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline replace corrected': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                          'amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                                          'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                          'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                          'amx_set_fw_iso(ctx, x_iso)',
                                          'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, None, '
                                          'None, stream)',
                                          'amx_set_fw_iso(ctx, None)',
                                          'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                          'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                          'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline replace fused': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                      'amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                      'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                      'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, '
                                      'stream)',
                                      'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                      'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline replace fused corrected': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                                'amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                                'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                'amx_set_fw_iso(ctx, x_iso)',
                                                'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, '
                                                'None, None, stream)',
                                                'amx_set_fw_iso(ctx, None)',
                                                'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline replace debias': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                       'amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                       'amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                                       'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                       'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                       'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, '
                                       'stream)',
                                       'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                       'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline replace debias corrected': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                                 'amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                                 'amx_prep_gather_device_f32(ctx, plan, d_img, int:1, float:0.0, y, mean_b0, stream)',
                                                 'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                 'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                                 'amx_set_fw_iso(ctx, x_iso)',
                                                 'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, '
                                                 'None, None, stream)',
                                                 'amx_set_fw_iso(ctx, None)',
                                                 'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                 'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                 'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline replace debias fused': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                             'amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                             'amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                             'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                             'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, '
                                             'None, stream)',
                                             'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                             'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline replace debias fused corrected': ['amx_prep_sanitize_device(ctx, plan, d_img, int:1, float:0.25, stream)',
                                                       'amx_prep_debias_device(ctx, plan, d_img, float:20.0, stream)',
                                                       'amx_prep_gather_directions_device_f32(ctx, plan, dti, d_img, int:1, float:0.0, y, mean_b0, dirs, '
                                                       'stream)',
                                                       'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                       'amx_set_fw_iso(ctx, x_iso)',
                                                       'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, '
                                                       'None, None, None, stream)',
                                                       'amx_set_fw_iso(ctx, None)',
                                                       'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                       'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                       'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline raw_dtype': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                  'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                  'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                  'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, stream)',
                                  'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                  'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline raw_dtype corrected': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                            'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                            'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                            'amx_set_fw_iso(ctx, x_iso)',
                                            'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, None, '
                                            'None, stream)',
                                            'amx_set_fw_iso(ctx, None)',
                                            'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                            'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                            'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline raw_dtype fused': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                        'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                        'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, '
                                        'stream)',
                                        'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                        'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline raw_dtype fused corrected': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                                  'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                                  'amx_set_fw_iso(ctx, x_iso)',
                                                  'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, '
                                                  'None, None, stream)',
                                                  'amx_set_fw_iso(ctx, None)',
                                                  'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                  'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                  'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline raw_dtype debias': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                         'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                         'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                         'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                         'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, '
                                         'stream)',
                                         'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                         'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline raw_dtype debias corrected': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                                   'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                                   'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                                   'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                                   'amx_set_fw_iso(ctx, x_iso)',
                                                   'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, '
                                                   'None, None, stream)',
                                                   'amx_set_fw_iso(ctx, None)',
                                                   'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                   'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                   'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline raw_dtype debias fused': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                               'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                               'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                               'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, '
                                               'None, stream)',
                                               'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                               'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline raw_dtype debias fused corrected': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:0, float:0.0, img, stream)',
                                                         'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                                         'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, '
                                                         'stream)',
                                                         'amx_set_fw_iso(ctx, x_iso)',
                                                         'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, '
                                                         'None, None, None, stream)',
                                                         'amx_set_fw_iso(ctx, None)',
                                                         'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                         'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                         'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline raw_dtype replace': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, stream)',
                                          'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                          'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                          'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                          'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, None, '
                                          'stream)',
                                          'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                          'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline raw_dtype replace corrected': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, stream)',
                                                    'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                                    'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                    'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                                    'amx_set_fw_iso(ctx, x_iso)',
                                                    'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, None, '
                                                    'None, None, stream)',
                                                    'amx_set_fw_iso(ctx, None)',
                                                    'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                    'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                    'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline raw_dtype replace fused': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, stream)',
                                                'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                                'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, None, '
                                                'None, stream)',
                                                'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline raw_dtype replace fused corrected': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, '
                                                          'stream)',
                                                          'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, '
                                                          'stream)',
                                                          'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                          'amx_set_fw_iso(ctx, x_iso)',
                                                          'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, '
                                                          'None, None, None, stream)',
                                                          'amx_set_fw_iso(ctx, None)',
                                                          'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                          'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                          'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline raw_dtype replace debias': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, stream)',
                                                 'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                                 'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                                 'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                 'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                                 'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, None, '
                                                 'None, None, stream)',
                                                 'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                 'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline raw_dtype replace debias corrected': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, '
                                                           'stream)',
                                                           'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                                           'amx_prep_gather_device_f32(ctx, plan, img, int:1, float:0.0, y, mean_b0, stream)',
                                                           'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                           'amx_dti_directions_device_f32(ctx, dti, y, int:6, dirs, stream)',
                                                           'amx_set_fw_iso(ctx, x_iso)',
                                                           'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:32, est, '
                                                           'None, None, None, stream)',
                                                           'amx_set_fw_iso(ctx, None)',
                                                           'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                           'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                           'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, stream)'],
 'freewater pipeline raw_dtype replace debias fused': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, img, stream)',
                                                       'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                                       'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, dirs, stream)',
                                                       'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                       'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, int:0, est, '
                                                       'None, None, None, stream)',
                                                       'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                       'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)'],
 'freewater pipeline raw_dtype replace debias fused corrected': ['amx_prep_ingest_device(ctx, plan, d_img, int:2, float:1.0, float:0.0, int:1, float:0.25, '
                                                                 'img, stream)',
                                                                 'amx_prep_debias_device(ctx, plan, img, float:20.0, stream)',
                                                                 'amx_prep_gather_directions_device_f32(ctx, plan, dti, img, int:1, float:0.0, y, mean_b0, '
                                                                 'dirs, stream)',
                                                                 'amx_sanitize_device_f32(ctx, y, int:42, int:1, float:0.25, stream)',
                                                                 'amx_set_fw_iso(ctx, x_iso)',
                                                                 'amx_freewater_fit_device_f32(ctx, lut, y, dirs, int:6, float:0.0, float:0.001, int:1, '
                                                                 'int:32, est, None, None, None, stream)',
                                                                 'amx_set_fw_iso(ctx, None)',
                                                                 'amx_prep_scatter_device(ctx, plan, est, int:4, maps, stream)',
                                                                 'amx_prep_scatter_device(ctx, plan, dirs, int:3, dirs_vol, stream)',
                                                                 'amx_prep_corrected_device(ctx, plan, lut, y, x_iso, mean_b0, None, int:0, corrected, '
                                                                 'stream)']}
