"""The image in its stored dtype (uint8 / int16 / uint16 / int32 / float32 / float64 + the NIfTI scaling): the numpy statement of the
value rule (tests/ingest_np.py) against hand-written cases, and what Evaluation.set_data does with such an image before anything
touches a GPU.  The kernel itself is held to ingest_np in tests/test_gpu_ingest.py."""
import numpy as np
import pytest

import badvox_np as B
import ingest_np as I
from amico_amd import synthetic as S


def f32bits(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


# ---------------------------------------------------------------- the helper against hand-written cases

def test_integer_extremes():
    out = I.convert(np.array([-32768, 32767, 0, -1], dtype=np.int16))
    assert out.dtype == np.float32 and out.tolist() == [-32768.0, 32767.0, 0.0, -1.0]
    assert I.convert(np.array([65535, 0], dtype=np.uint16)).tolist() == [65535.0, 0.0]
    assert I.convert(np.array([255], dtype=np.uint8)).tolist() == [255.0]


def test_int32_rounds_to_nearest_even():
    raw = np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    out = I.convert(raw)
    # 2^24 + 1 is half way between 2^24 and 2^24 + 2: to the even mantissa, 2^24; 2^24 + 3 -> 2^24 + 4
    assert out.tolist() == [16777216.0, 16777220.0, -16777216.0, 2147483648.0, -2147483648.0]


def test_float64_edges():
    raw = np.array([1e39, -1e39, -1e-46, 1e-46, 1e-40, np.nan, np.inf, -np.inf, -0.0, 3.4028235677973366e38], dtype=np.float64)
    out = I.convert(raw)
    assert np.isposinf(out[0]) and np.isneginf(out[1])                                # beyond float32's range
    assert f32bits(out[2]) == 0x80000000 and f32bits(out[3]) == 0                     # below half the smallest denormal: +-0, sign kept
    assert f32bits(out[4]) == f32bits(np.float32(1e-40)) != 0 and out[4] < np.finfo(np.float32).tiny    # a float32 denormal
    assert np.isnan(out[5]) and np.isposinf(out[6]) and np.isneginf(out[7]) and f32bits(out[8]) == 0x80000000
    assert np.isposinf(out[9])                                                        # half an ulp above float32's largest: a tie, to even = Inf
    img, n = I.ingest(raw)
    assert n == 6 and np.array_equal(B.bits(img), B.bits(out))
    img, n = I.ingest(raw, replace=7.5)
    assert n == 6 and np.isfinite(img).all() and (img == 7.5).sum() == 6
    keep = np.isfinite(out)
    assert np.array_equal(B.bits(img[keep]), B.bits(out[keep]))                       # finite elements keep their bits, -0.0 and denormals too


def test_scaling_on_raw_zero_and_others():
    assert I.convert(np.array([0], dtype=np.int16), (-2.5, 1024)).tolist() == [1024.0]
    assert I.convert(np.array([2, -4], dtype=np.int16), (-2.5, 1024)).tolist() == [1019.0, 1034.0]
    # product and sum in float64, ONE narrowing: 1000 * 0.0125 - 3.5 = 9.0 exactly in float64; float32(0.0125) * 1000 would not give it
    assert I.convert(np.array([1000], dtype=np.uint16), (0.0125, -3.5)).tolist() == [9.0]
    out = I.convert(np.array([1.5, np.nan], dtype=np.float32), (2.0, 1.0))
    assert out[0] == 4.0 and np.isnan(out[1])


def test_fused_multiply_add_would_differ():
    """the case the kernel's `contract(off)` is there for: searched, and asserted to separate the two forms"""
    r, slope, inter = I.fma_sensitive_case()
    assert -32768 <= r <= 32767
    two = I.convert(np.array([r], dtype=np.int16), (slope, inter))[0]
    fused = I.fma_float32(r, slope, inter)
    assert f32bits(two) != f32bits(fused)
    assert f32bits(two) == f32bits(np.float32(np.float64(r) * slope + inter))
    assert abs(int(f32bits(two)) - int(f32bits(fused))) == 1                          # neighbours: a rounding difference, nothing else


def test_same_bits_helper():
    a = np.array([1.0, np.nan, -0.0], dtype=np.float32)
    b = a.copy()
    b.view(np.uint32)[1] = 0x7fc00001                                                 # another payload: still the same value rule
    assert I.same_bits(a, b)
    assert not I.same_bits(a, np.array([1.0, np.nan, 0.0], dtype=np.float32))
    assert not I.same_bits(a, np.array([1.0, 2.0, -0.0], dtype=np.float32))


# ---------------------------------------------------------------- set_data, before any context exists

def small_case(dtype=np.int16, order='F'):
    sch = S.make_scheme(seed=0)
    raw = np.asarray(np.random.default_rng(1).integers(0, 4000, size=(3, 2, 2, sch.nS)).astype(dtype), order=order)
    return raw, sch, np.ones((3, 2, 2), dtype=np.uint8)


@pytest.mark.parametrize('scaling', [(float('nan'), 0.0), (1.0, float('inf')), (0, 0), (0.0, 5.0), ('2', 0), (1.0,), 3.0, (1, 2, 3),
                                     (np.float32('inf'), 0)])
def test_set_data_refuses_a_bad_scaling(scaling):
    """on the host, before a context is made: this passes on a machine without a GPU (without the feature set_data has no such
    argument and this is a TypeError)"""
    import amico_amd
    raw, sch, mask = small_case()
    ae = amico_amd.Evaluation()
    with pytest.raises(ValueError, match='scaling'):
        ae.set_data(raw, sch, mask, scaling=scaling)
    assert ae.niiDWI_img is None


@pytest.mark.parametrize('scaling, want', [(None, None), ((None, None), None), ((None, 3.0), None), ((1, 0), None), ((1.0, None), None),
                                           ((2, None), (2.0, 0.0)), ((np.float32(0.5), np.int16(-3)), (0.5, -3.0))])
def test_scalings_that_pass(scaling, want):
    from amico_amd import prep
    assert prep.check_scaling(scaling) == want


def test_streamable_layouts():
    from amico_amd import prep
    raw, _, _ = small_case()
    assert prep.streamable(raw) and prep.streamable(np.ascontiguousarray(raw)) and prep.streamable(raw.transpose(3, 0, 1, 2).copy().transpose(1, 2, 3, 0))
    assert not prep.streamable(raw[:, :, :, ::2]) and not prep.streamable(raw[1:]) and not prep.streamable(raw[::-1])
    assert not prep.streamable(raw.astype(np.int64)) and not prep.streamable(raw.astype(np.float16)) and not prep.streamable(raw[0])
    one = np.zeros((3, 1, 2, 5), dtype=np.int16)
    odd = np.lib.stride_tricks.as_strided(one, shape=one.shape, strides=(one.strides[0], 998, one.strides[2], one.strides[3]))
    assert prep.streamable(one) and prep.streamable(odd)                             # the stride of an axis of extent 1 does not count


class _NoGpuPreparation:
    """stands in for SignalPreparation (which makes a context): set_data's own work is what these tests look at"""
    last = None

    def __init__(self, scheme, img_like, mask, **kw):
        type(self).last = (img_like, kw)


@pytest.mark.parametrize('dtype', [np.int16, np.uint16, np.float64])
def test_set_data_keeps_the_stored_array(monkeypatch, dtype):
    import amico_amd
    from amico_amd import core
    monkeypatch.setattr(core._prep, 'SignalPreparation', _NoGpuPreparation)
    raw, sch, mask = small_case(dtype)
    scaling = (0.0125, -3.5) if dtype == np.int16 else None
    ae = amico_amd.Evaluation()
    ae.set_data(raw, sch, mask, scaling=scaling)
    planned_on, kw = _NoGpuPreparation.last
    assert planned_on is raw and ae._raw is raw and kw['scaling'] == scaling          # the plan is made on the stored array itself
    assert ae._img32 is None                                                          # no float32 copy was made ...
    assert ae.get_config('dim') == raw.shape[:3]
    img = ae.niiDWI_img                                                               # ... until it is asked for
    assert img.dtype == np.float32 and img.strides == tuple(s // raw.itemsize * 4 for s in raw.strides)
    assert np.array_equal(B.bits(img), B.bits(I.convert(raw, scaling)))
    assert ae.niiDWI_img is img                                                       # cached
    # assigning keeps working, and takes the place of the stored array
    other = np.zeros(raw.shape, dtype=np.float32)
    ae.niiDWI_img = other
    assert ae.niiDWI_img is other and ae._raw is None


def test_set_data_float32_and_unstreamable_inputs_take_the_host_route(monkeypatch):
    import amico_amd
    from amico_amd import core
    monkeypatch.setattr(core._prep, 'SignalPreparation', _NoGpuPreparation)
    raw, sch, mask = small_case(np.float32)
    ae = amico_amd.Evaluation()
    ae.set_data(raw, sch, mask)
    assert ae._raw is None and ae.niiDWI_img is raw and _NoGpuPreparation.last[0] is raw and _NoGpuPreparation.last[1]['scaling'] is None
    ae.set_data(raw, sch, mask, scaling=(1.0, 0.0))                                   # the identity is no scaling
    assert ae._raw is None and ae.niiDWI_img is raw
    ae.set_data(raw, sch, mask, scaling=(2.0, 1.0))                                   # float32 WITH a scaling is converted on the GPU
    assert ae._raw is raw and ae._img32 is None
    assert np.array_equal(ae.niiDWI_img, I.convert(raw, (2.0, 1.0)))
    # a dtype the kernel does not take, and a view with gaps: numpy's expression, on the host, now
    big, _, _ = small_case(np.int64)
    ae.set_data(big, sch, mask, scaling=(0.5, 1.0))
    assert ae._raw is None and np.array_equal(B.bits(ae._img32), B.bits(I.convert(big, (0.5, 1.0))))
    assert _NoGpuPreparation.last[0] is ae._img32 and _NoGpuPreparation.last[1]['scaling'] is None
    wide = np.zeros((3, 2, 2, 2 * sch.nS), dtype=np.int16)
    wide[...] = np.arange(2 * sch.nS)
    ae.set_data(wide[..., ::2], sch, mask, scaling=(0.5, 1.0))
    assert ae._raw is None and np.array_equal(ae._img32, I.convert(wide[..., ::2], (0.5, 1.0)))
    # the geometry checks and their texts are as they were
    with pytest.raises(ValueError, match='DWI file is not a 4D image'):
        ae.set_data(raw[0].astype(np.int16), sch, mask)
    with pytest.raises(ValueError, match='Scheme does not match with DWI data'):
        ae.set_data(raw[..., :-1].astype(np.int16), sch, mask)
    with pytest.raises(ValueError, match='MASK geometry does not match with DWI data'):
        ae.set_data(raw.astype(np.int16), sch, mask[1:])


def test_fit_without_data_still_says_so():
    import amico_amd
    with pytest.raises(RuntimeError, match='Data not loaded'):
        amico_amd.Evaluation().fit()
