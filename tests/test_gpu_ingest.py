"""The image in its stored dtype on the GPU (amx_prep_ingest*): the kernel against tests/ingest_np.py bit for bit, Evaluation.fit() on
int16 / uint16 / float64 images against Evaluation.fit() on the float32 image numpy makes of them (every array of RESULTS equal on
bits), the kernels each route enqueues, and the device-resident pipelines.

Bit for bit means: equal as uint32 outside NaN positions, NaN positions coincide (ingest_np.same_bits).  Shapes are small on purpose:
1 155 elements (not a multiple of 8, under one workgroup) and 98 605 (odd, many workgroups)."""
import functools
import os
import warnings

import numpy as np
import pytest

import badvox_np as B
import ingest_np as I

pytestmark = pytest.mark.gpu

SCALINGS = [None, (0.0125, -3.5), (-2.5, 1024)]
VOLUMES = [(5, 7, 3, 11), (37, 41, 5, 13)]
F32_MAX = float(np.finfo(np.float32).max)


@functools.lru_cache(maxsize=None)
def _htable():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'htable500.npz'), allow_pickle=False))


def plain_scheme(nS):
    from amico_amd import synthetic as S
    b = np.where(np.arange(nS) % 5 == 0, 0.0, 1000.0)
    return S.SimpleScheme(np.column_stack([np.tile([1.0, 0.0, 0.0], (nS, 1)), b]))


def raw_values(dtype, n, seed):
    """`n` values of `dtype` that reach every corner of the value rule"""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind in 'iu':
        info = np.iinfo(dtype)
        a = rng.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64)
        edge = [info.min, info.max, 0, 1, info.max - 1]
        if dtype == np.int32:
            edge += [2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 2 ** 25 + 2, 2 ** 31 - 65, 2 ** 31 - 64]      # ties and near-ties of the rounding
        a[rng.choice(n, len(edge), replace=False)] = edge
        return a.astype(dtype)
    a = (rng.standard_normal(n) * 1000.0).astype(dtype)
    edge = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, F32_MAX, -F32_MAX, 1.17549435e-38]
    if dtype == np.float64:
        edge += [1e39, -1e39, 1e300, -1e-46, 1e-46, 7.1e-46, 5e-324, 3.4028235677973366e38, 3.4028235677973362e38, 1.0 + 2.0 ** -24,
                 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, 2.0 ** -149 * 1.5, 2.0 ** -149 * 2.5, 2.0 ** -127 * (1 + 2.0 ** -23)]
    edge = np.array(edge, dtype=dtype).repeat(3)
    a[rng.choice(n, len(edge), replace=False)] = edge
    return a


def flat_of(a):
    """the elements of a C- or Fortran-ordered array in memory order"""
    return np.lib.stride_tricks.as_strided(a, shape=(a.size,), strides=(a.itemsize,))


def run_kernel(plan, raw, scaling, replace, raw_offset=0, out_offset=0):
    """-> (float32 image in memory order, count); the buffers start `raw_offset` elements / `out_offset` floats behind a 16-byte
    boundary, and the words either side of the output hold a pattern that must survive"""
    import torch
    ctx = plan.ctx
    src = flat_of(raw)
    pad = 16 // raw.itemsize
    host = np.zeros(src.size + 2 * pad, dtype=raw.dtype)
    host[raw_offset:raw_offset + src.size] = src
    d_raw = torch.from_numpy(host.view(np.uint8)).to('cuda')
    assert d_raw.data_ptr() % 16 == 0
    d_out = torch.full((src.size + 8,), -7.0, dtype=torch.float32, device='cuda')
    assert d_out.data_ptr() % 16 == 0
    plan.ingest_device(d_raw.data_ptr() + raw_offset * raw.itemsize, raw.dtype, d_out.data_ptr() + 4 * out_offset, scaling, replace)
    count = ctx.sanitize_last()
    out = d_out.cpu().numpy()
    assert (out[:out_offset] == -7.0).all() and (out[out_offset + src.size:] == -7.0).all()
    return out[out_offset:out_offset + src.size], count


# ---------------------------------------------------------------- 1. the kernel, bit for bit

@pytest.mark.parametrize('dtype', I.DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_matches_numpy(dtype):
    from amico_amd import prep
    seen_bad = 0
    for shape in VOLUMES:
        for order in ('C', 'F'):
            raw = np.asarray(raw_values(dtype, int(np.prod(shape)), seed=shape[0]).reshape(shape), order=order)
            mask = np.random.default_rng(2).choice(np.array([0, 1, 1], dtype=np.uint8), size=shape[:3])
            sp = prep.SignalPreparation(plain_scheme(shape[3]), raw, mask, do_normalize=False)
            assert sp._plan.strides == tuple(s // raw.itemsize for s in raw.strides)
            for scaling in SCALINGS:
                want, want_n = I.ingest(raw, scaling)
                got, n = run_kernel(sp._plan, raw, scaling, None)
                assert n == want_n, (shape, order, scaling)
                assert I.same_bits(got, flat_of(want)), (shape, order, scaling)
                want_r, _ = I.ingest(raw, scaling, 123.5)
                got_r, n = run_kernel(sp._plan, raw, scaling, 123.5)
                assert n == want_n and np.isfinite(got_r).all()
                assert np.array_equal(B.bits(got_r), B.bits(flat_of(want_r))), (shape, order, scaling)      # no NaN left: plain bits
                keep = np.isfinite(flat_of(want))
                assert np.array_equal(B.bits(got_r[keep]), B.bits(got[keep]))          # finite elements keep their bits
                seen_bad += want_n
                if np.dtype(dtype).kind in 'iu':
                    assert want_n == 0                                                # clean data: a count of 0
    if np.dtype(dtype).kind == 'f':
        assert seen_bad > 0
    # the host-buffer twin, once
    img, n = sp._plan.ingest(raw, SCALINGS[1], 0.0)
    want, want_n = I.ingest(raw, SCALINGS[1], 0.0)
    assert n == want_n and img.strides == want.strides and np.array_equal(B.bits(img), B.bits(want))


@pytest.mark.parametrize('dtype', I.DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_on_buffers_off_the_16_byte_boundary(dtype):
    """the raw block one element behind a 16-byte boundary; the float32 block one and three floats behind one (head elements)"""
    from amico_amd import prep
    for shape in VOLUMES:
        raw = raw_values(dtype, int(np.prod(shape)), seed=11).reshape(shape)
        sp = prep.SignalPreparation(plain_scheme(shape[3]), raw, np.ones(shape[:3], dtype=np.uint8), do_normalize=False)
        for scaling in (None, SCALINGS[1]):
            want, want_n = I.ingest(raw, scaling, -2.0)
            for raw_off, out_off in ((1, 0), (0, 1), (1, 3), (3, 2)):
                got, n = run_kernel(sp._plan, raw, scaling, -2.0, raw_off, out_off)
                assert n == want_n and np.array_equal(B.bits(got), B.bits(flat_of(want))), (shape, scaling, raw_off, out_off)


def test_kernel_does_not_fuse_the_multiply_add():
    """the sample ingest_np searches: float32(fma(r, slope, inter)) is the NEIGHBOUR of what numpy gives"""
    from amico_amd import prep
    r, slope, inter = I.fma_sensitive_case()
    shape = VOLUMES[0]
    raw = np.full(shape, r, dtype=np.int16)
    want = I.convert(raw, (slope, inter))
    assert want.view(np.uint32).ravel()[0] != I.fma_float32(r, slope, inter).view(np.uint32)
    sp = prep.SignalPreparation(plain_scheme(shape[3]), raw, np.ones(shape[:3], dtype=np.uint8), do_normalize=False)
    for dtype in (np.int16, np.int32, np.float32, np.float64):
        got, n = run_kernel(sp._plan, raw.astype(dtype), (slope, inter), None)
        assert n == 0 and np.array_equal(B.bits(got), B.bits(flat_of(want))), np.dtype(dtype).name


def test_bad_arguments_are_refused_with_a_message():
    import torch
    from amico_amd import _capi, prep
    shape = VOLUMES[0]
    raw = raw_values(np.int16, int(np.prod(shape)), seed=3).reshape(shape)
    sp = prep.SignalPreparation(plain_scheme(shape[3]), raw, np.ones(shape[:3], dtype=np.uint8), do_normalize=False)
    ctx, plan, L = sp.ctx, sp._plan, _capi.lib()
    d_raw = torch.from_numpy(raw).to('cuda')
    d_out = torch.zeros(raw.size, dtype=torch.float32, device='cuda')
    t = _capi.RAW_DTYPES[np.dtype(np.int16)]

    def call(dtype=t, slope=1.0, inter=0.0, replace=0, value=0.0, p=plan._h, raw_ptr=d_raw.data_ptr(), out_ptr=d_out.data_ptr()):
        rc = L.amx_prep_ingest_device(ctx._h, p, raw_ptr, dtype, slope, inter, replace, value, out_ptr, None)
        return rc, L.amx_last_error(ctx._h).decode()
    for kw, text in (({'slope': float('nan')}, 'slope and inter must be finite'), ({'slope': float('inf')}, 'slope and inter must be finite'),
                     ({'inter': float('-inf')}, 'slope and inter must be finite'), ({'replace': 1, 'value': float('nan')}, 'replacement value must be finite'),
                     ({'replace': 1, 'value': float('inf')}, 'replacement value must be finite'), ({'dtype': 0}, 'raw_dtype'), ({'dtype': 7}, 'raw_dtype'),
                     ({'raw_ptr': d_raw.data_ptr() + 1}, 'not aligned'), ({'out_ptr': d_out.data_ptr() + 2}, 'not aligned'),
                     ({'raw_ptr': d_out.data_ptr() + 64}, 'overlap'), ({'raw_ptr': None}, 'null')):
        rc, msg = call(**kw)
        assert rc == _capi.AMX_E_BADARG and text in msg, (kw, rc, msg)
    assert call(replace=0, value=float('nan'))[0] == _capi.AMX_OK                     # the value is not looked at when nothing is replaced
    assert ctx.sanitize_last() == 0
    ctx.sync()
    with pytest.raises(ValueError, match='finite'):
        plan.ingest_device(d_raw.data_ptr(), np.int16, d_out.data_ptr(), (float('nan'), 0.0))
    # a view with gaps cannot be streamed: refused with a message (Python then converts on the host)
    wide = np.zeros(shape[:3] + (2 * shape[3],), dtype=np.float32)
    gaps = prep.SignalPreparation(plain_scheme(shape[3]), wide[..., ::2], np.ones(shape[:3], dtype=np.uint8), do_normalize=False)
    d_wide = torch.zeros(wide.size, dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError, match='not a permutation of a contiguous block'):
        gaps._plan.ingest_device(d_raw.data_ptr(), np.int16, d_wide.data_ptr())
    with pytest.raises(ValueError, match='DWI image must be a 4D float32 array'):
        prep.SignalPreparation(plain_scheme(shape[3]), raw[:, ::-1], np.ones(shape[:3], dtype=np.uint8))       # int16 that cannot be streamed


# ---------------------------------------------------------------- 2. Evaluation.fit(), end to end

SHAPE = (12, 10, 6)


@functools.lru_cache(maxsize=None)
def scene(model):
    """dictionary, scheme, mask (about 2/3 of 12 x 10 x 6) and the noise-free signals in scanner units (float64, order F), made once"""
    from amico_amd import synthetic as S
    h = _htable()
    n = int(np.prod(SHAPE))
    mask = (np.random.default_rng(4).uniform(size=SHAPE) < 2.0 / 3.0).astype(np.uint8)
    if model == 'NODDI':
        sch = S.make_scheme(seed=0)
        assert sch.nS == 99
        K = S.noddi_kernels(sch, h['dirs'])
        y, _ = S.noddi_signals(n, K, h['htable'], sch, seed=6)
        kernels = (K, h['htable'])
    elif model == 'FreeWater':
        sch = S.make_scheme(5, ((1000.0, 60),), seed=3)
        K = S.freewater_kernels(sch, h['dirs'])
        y, _ = S.freewater_signals(n, K, h['htable'], sch, seed=8)
        kernels = (K, h['htable'])
    else:
        sch = S.make_sandi_scheme(ndir_per_shell=24, n_b0=4)
        avg = S.directional_average_scheme(sch)
        ya = S.sandi_signals(n, S.sandi_kernels(avg)[0], avg, seed=3)
        y = np.ones((n, sch.nS))
        for k, sh in enumerate(sorted(sch.shells, key=lambda s: s['b'])):
            y[:, sh['idx']] = ya[:, k + 1:k + 2] * (1.0 + 0.05 * np.random.default_rng(k).standard_normal((n, len(sh['idx']))))
        kernels = None
    sig = np.asfortranarray(y.reshape(SHAPE + (-1,)) * 800.0)
    sig.setflags(write=False)
    return dict(model=model, sch=sch, mask=mask, kernels=kernels, sig=sig)


def stored(sc, kind):
    """the scene's image as a scanner would have stored it -> (array, scaling)"""
    sig = sc['sig']
    if kind == 'int16':
        scaling = (0.05, -3.5)
        raw = np.rint((sig - scaling[1]) / scaling[0])
        assert raw.max() < 32767 and raw.min() >= 0
        return raw.astype(np.int16), scaling
    if kind == 'uint16':
        raw = np.rint(sig * 64.0)
        assert 32767 < raw.max() < 65535
        return raw.astype(np.uint16), None
    return np.array(sig, order='F'), None               # float64: what nibabel's get_fdata() hands out


def evaluation(sc, dwi, scaling=None, replace=None, config=()):
    import amico_amd
    from amico_amd import synthetic as S
    ae = amico_amd.Evaluation()
    for k, v in config:
        ae.set_config(k, v)
    ae.set_data(dwi, sc['sch'], sc['mask'], replace_bad_voxels=replace, scaling=scaling)
    ae.set_model(sc['model'])
    if sc['model'] == 'SANDI':
        ae.set_kernels(S.sandi_kernels(ae.scheme)[0])
    else:
        ae.set_kernels(*sc['kernels'])
    return ae


def same_results(a, b):
    assert set(a.RESULTS) == set(b.RESULTS) and 'MAPs' in a.RESULTS
    for k in a.RESULTS:
        assert a.RESULTS[k].dtype == b.RESULTS[k].dtype and np.array_equal(B.bits(a.RESULTS[k]), B.bits(b.RESULTS[k])), k
    for k in ('bad_samples_raw', 'bad_samples_preprocessed'):
        assert a.get_config(k) == b.get_config(k), k


def fit_both(sc, raw, scaling=None, replace=None, config=()):
    """-> (fit on the stored array, fit on the float32 array numpy makes of it)"""
    ae = evaluation(sc, raw, scaling, replace, config)
    assert ae._raw is raw and ae._img32 is None
    ae.fit()
    assert ae._img32 is None                           # fit() never made the float32 image on the host
    ref = evaluation(sc, I.convert(raw, scaling), None, replace, config)
    assert ref._raw is None
    ref.fit()
    same_results(ae, ref)
    assert np.array_equal(ae.y, ref.y)
    assert np.array_equal(B.bits(ae.niiDWI_img), B.bits(ref.niiDWI_img))
    return ae, ref


@pytest.mark.parametrize('kind', ['int16', 'uint16', 'float64'])
def test_evaluation_noddi_on_the_stored_image(kind):
    sc = scene('NODDI')
    raw, scaling = stored(sc, kind)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ae, ref = fit_both(sc, raw, scaling)
    assert ae.get_config('bad_samples_raw') == 0 and ae.RESULTS['MAPs'].shape == SHAPE + (3,) and ae.RESULTS['MAPs'][sc['mask'] == 1].any()


def test_evaluation_freewater_corrected_dwi_on_int16():
    sc = scene('FreeWater')
    raw, scaling = stored(sc, 'int16')
    ae, _ = fit_both(sc, raw, scaling, config=(('doSaveCorrectedDWI', True), ('doKeepb0Intact', True)))
    assert ae.RESULTS['DWI_corrected'].shape == raw.shape and ae.RESULTS['DWI_corrected'][sc['mask'] == 1].any()


def test_evaluation_sandi_directional_average_on_uint16():
    sc = scene('SANDI')
    raw, scaling = stored(sc, 'uint16')
    ae, _ = fit_both(sc, raw, scaling, config=(('doDirectionalAverage', True),))
    assert ae.scheme.nS == 6 and 'DIRs' not in ae.RESULTS


def test_evaluation_debias_on_int16():
    sc = scene('NODDI')
    raw, scaling = stored(sc, 'int16')
    ae, _ = fit_both(sc, raw, scaling, config=(('doDebiasSignal', True), ('DWI-SNR', 25.0)))
    assert ae.get_config('debias_unconverged') == 0


def float64_with_overflow(sc):
    raw, _ = stored(sc, 'float64')
    inside, outside = np.argwhere(sc['mask'] == 1)[7], np.argwhere(sc['mask'] == 0)[2]
    raw[inside[0], inside[1], inside[2], 17] = 1e39          # finite as float64, +Inf as float32
    raw[outside[0], outside[1], outside[2], 3] = -1e39
    raw[inside[0], inside[1], inside[2], 40] = np.nan
    assert np.isfinite(raw).sum() == raw.size - 1
    return raw


def test_same_refusal_when_a_float64_sample_overflows_float32():
    sc = scene('NODDI')
    raw = float64_with_overflow(sc)
    texts = []
    for dwi in (raw, I.convert(raw)):
        ae = evaluation(sc, dwi)
        with pytest.raises(RuntimeError, match='Nan or Inf values in the raw signal') as err:
            ae.fit()
        assert ae.RESULTS is None and ae._dev is None and ae.get_config('bad_samples_raw') == 3
        texts.append(str(err.value))
    assert texts[0] == texts[1]


def test_same_warning_and_maps_with_a_replacement_value():
    sc = scene('NODDI')
    raw = float64_with_overflow(sc)
    msgs = []
    fits = []
    for dwi in (raw, I.convert(raw)):
        ae = evaluation(sc, dwi, replace=0)
        with pytest.warns(UserWarning, match='Nan or Inf values in the raw signal. They will be replaced with: 0') as rec:
            ae.fit()
        msgs.append(sorted(str(w.message) for w in rec))
        fits.append(ae)
    assert msgs[0] == msgs[1]
    same_results(*fits)
    assert fits[0].get_config('bad_samples_raw') == 3 and np.isfinite(fits[0].RESULTS['MAPs']).all()
    assert B.count(fits[0].niiDWI_img) == 3                 # the host image keeps what the stored values convert to


# ---------------------------------------------------------------- 3. which kernels each route enqueues

def prep_path(ae):
    """the kernels fit() enqueues AHEAD of the model fit (which starts amx_last_path over), on a fresh context"""
    ctx = ae._prep.ctx
    before = ctx.last_path()
    seen = []
    inner = ae.model.fit

    def spy(ev):
        seen.append(ctx.last_path())
        return inner(ev)
    ae.model.fit = spy
    ae.fit()
    assert len(seen) == 1 and seen[0].startswith(before) and len(seen[0]) < 1400       # (amx_last_path keeps 1 500 characters)
    return seen[0][len(before):].removeprefix(' -> ')


def test_paths_of_the_two_routes():
    import amico_amd
    sc = scene('NODDI')
    raw, scaling = stored(sc, 'int16')
    amico_amd.reset_context()
    try:
        p_raw = prep_path(evaluation(sc, raw, scaling))
        amico_amd.reset_context()
        p_f32 = prep_path(evaluation(sc, I.convert(raw, scaling)))
    finally:
        amico_amd.reset_context()
    # a stored image: the ingest kernel first, and ONE scan -- that of y -- behind it
    assert p_raw.startswith('k_ingest<i16,scaled> -> '), p_raw
    assert p_raw.count('k_sanitize') == 1 and p_raw.count('k_ingest') == 1, p_raw
    # float32: the sequence as it was -- scan of the image, ..., scan of y -- and no ingest
    assert 'k_ingest' not in p_f32 and p_f32.startswith('k_sanitize_flat<f32> -> ') and p_f32.count('k_sanitize_flat<f32>') == 2, p_f32
    assert p_raw.replace('k_ingest<i16,scaled>', 'k_sanitize_flat<f32>', 1) == p_f32


# ---------------------------------------------------------------- 4. the device-resident chains

def dev_bytes(a):
    import torch
    return torch.from_numpy(flat_of(a).view(np.uint8).copy()).to('cuda:0')


def test_noddi_volume_pipeline_on_an_int16_tensor():
    import torch
    from amico_amd import pipeline
    sc = scene('NODDI')
    raw, scaling = stored(sc, 'int16')
    img = I.convert(raw, scaling)
    K, ht = sc['kernels']
    pl = pipeline.NoddiVolumePipeline(sc['sch'], raw, sc['mask'], K, ht, raw_dtype=np.int16, scaling=scaling)
    d_raw = torch.from_numpy(flat_of(raw).copy()).to('cuda:0')
    assert d_raw.dtype == torch.int16
    maps, dirs = (t.cpu().numpy() for t in pl.run(d_raw))
    assert pl.bad_samples == 0 and np.array_equal(d_raw.cpu().numpy(), flat_of(raw))      # the stored tensor is left as it is
    assert I.same_bits(pl.img.cpu().numpy(), flat_of(img))
    plain = pipeline.NoddiVolumePipeline(sc['sch'], img, sc['mask'], K, ht)
    maps0, dirs0 = (t.cpu().numpy() for t in plain.run(torch.from_numpy(flat_of(img).copy()).to('cuda:0')))
    assert plain.raw_dtype is None and plain.img is None
    assert np.array_equal(B.bits(maps), B.bits(maps0)) and np.array_equal(B.bits(dirs), B.bits(dirs0)) and maps[sc['mask'] == 1].any()
    # float64 with samples float32 cannot hold, replaced by the chain: the counts and maps of the float32 chain on numpy's image
    bad = float64_with_overflow(sc)
    pr = pipeline.NoddiVolumePipeline(sc['sch'], bad, sc['mask'], K, ht, replace_bad_voxels=0.0)
    assert pr.raw_dtype == np.float64
    maps_r, _ = pr.run(dev_bytes(bad))
    p0 = pipeline.NoddiVolumePipeline(sc['sch'], I.convert(bad), sc['mask'], K, ht, replace_bad_voxels=0.0)
    maps_0, _ = p0.run(torch.from_numpy(flat_of(I.convert(bad)).copy()).to('cuda:0'))
    assert pr.bad_samples == p0.bad_samples == 3 and pr.bad_samples_preprocessed == p0.bad_samples_preprocessed
    assert np.array_equal(B.bits(maps_r.cpu().numpy()), B.bits(maps_0.cpu().numpy()))


def test_freewater_volume_pipeline_on_a_uint16_tensor():
    import torch
    from amico_amd import pipeline
    sc = scene('FreeWater')
    raw, scaling = stored(sc, 'uint16')
    img = I.convert(raw, scaling)
    K, ht = sc['kernels']
    pl = pipeline.FreeWaterVolumePipeline(sc['sch'], raw, sc['mask'], K, ht, corrected=True, raw_dtype=np.uint16)
    maps, dirs = pl.run(dev_bytes(raw))
    plain = pipeline.FreeWaterVolumePipeline(sc['sch'], img, sc['mask'], K, ht, corrected=True)
    maps0, dirs0 = plain.run(torch.from_numpy(flat_of(img).copy()).to('cuda:0'))
    for a, b in ((maps, maps0), (dirs, dirs0), (pl.corrected, plain.corrected)):
        assert np.array_equal(B.bits(a.cpu().numpy()), B.bits(b.cpu().numpy()))
    assert pl.bad_samples == 0 and plain.bad_samples is None
