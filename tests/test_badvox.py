"""replace_bad_voxels without a GPU: the numpy model of core.py:152-158 / 270-276 (tests/badvox_np.py) on hand cases, and the argument
checks of Evaluation.set_data / SignalPreparation, which must fail on the host before a context is created or anything is uploaded."""
import warnings

import numpy as np
import pytest

import badvox_np as B
from amico_amd import synthetic as S

F32_MAX = np.finfo(np.float32).max
DENORMAL = np.float32(1e-45)


def hand_case(dtype):
    return np.array([1.0, np.nan, -0.0, np.inf, DENORMAL, -np.inf, F32_MAX, -DENORMAL, 0.0, -F32_MAX, -np.nan, 2.5], dtype=dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_model_counts_nan_and_both_infinities_only(dtype):
    a = hand_case(dtype)
    assert B.count(a) == 4
    assert np.array_equal(np.flatnonzero(B.bad(a)), [1, 3, 5, 10])
    assert B.count(np.array([-0.0, DENORMAL, F32_MAX, -F32_MAX], dtype=dtype)) == 0
    assert B.count(np.zeros((0, 3), dtype=dtype)) == 0


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('r', [0.0, 123.5, -7.0])
def test_model_replaces_exactly_the_bad_samples(dtype, r):
    a = hand_case(dtype)
    out = B.replace(a, r)
    assert out.dtype == a.dtype and out is not a and np.isnan(a[1])          # a copy: the input keeps its NaN
    isbad = B.bad(a)
    assert np.array_equal(B.bits(out[isbad]), B.bits(np.full(4, r, dtype=dtype)))
    # every finite element keeps its bits: -0.0 stays -0.0, denormals stay denormal, the largest float32 stays
    assert np.array_equal(B.bits(out[~isbad]), B.bits(a[~isbad]))
    assert np.signbit(out[2]) and out[4] == DENORMAL and out[6] == F32_MAX
    assert B.count(out) == 0


def _capi_value(r):
    from amico_amd import _capi
    return _capi._replacement(r, np.float32)


def test_model_rounds_the_value_once_to_the_image_type():
    a = np.array([np.nan, 1.0], dtype=np.float32)
    out = B.replace(a, 0.1)                                  # 0.1 is no float32: the image gets float32(0.1)
    assert out[0] == np.float32(0.1) and float(out[0]) != 0.1
    r = 1.0 + 2.0 ** -24 + 2.0 ** -50                        # a float64 just above the midpoint of two float32: rounds up, to nearest
    assert B.replace(a, r)[0] == np.float32(1.0 + 2.0 ** -23) and _capi_value(r) == float(np.float32(1.0 + 2.0 ** -23))
    from amico_amd import _capi
    assert _capi._replacement(0.1, np.float32) == float(np.float32(0.1))
    assert _capi._replacement(0.1, np.float64) == 0.1
    assert _capi._replacement(None, np.float32) == 0.0


def test_model_keeps_the_memory_order():
    img = np.asfortranarray(np.arange(24, dtype=np.float32).reshape(2, 3, 4))
    img[1, 2, 3] = np.inf
    out = B.replace(img, 0.0)
    assert out.strides == img.strides and out[1, 2, 3] == 0.0 and B.count(img) == 1


def small_case():
    sch = S.make_scheme(seed=0)
    img = np.full((3, 2, 2, sch.nS), 100.0, dtype=np.float32)
    mask = np.ones((3, 2, 2), dtype=np.uint8)
    return img, sch, mask


@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf'), 'x', '0', 1e39, 10 ** 400, [0.0], np.float32('nan')])
def test_set_data_refuses_a_value_that_is_not_a_finite_number(value):
    """on the host, before a context is made: this passes on a machine without a GPU (on the code without the feature set_data has no
    such argument and this is a TypeError)"""
    import amico_amd
    img, sch, mask = small_case()
    ae = amico_amd.Evaluation()
    with pytest.raises(ValueError, match='replace_bad_voxels'):
        ae.set_data(img, sch, mask, replace_bad_voxels=value)
    assert ae.niiDWI_img is None and ae.get_config('replace_bad_voxels') is None


@pytest.mark.parametrize('value', [float('nan'), float('inf'), 'x'])
def test_signal_preparation_refuses_it_too(value):
    from amico_amd import prep
    img, sch, mask = small_case()
    with pytest.raises(ValueError, match='replace_bad_voxels'):
        prep.SignalPreparation(sch, img, mask, replace_bad_voxels=value)
    with pytest.raises(ValueError, match='replace_bad_voxels'):
        prep.check_replace_bad_voxels(value)


@pytest.mark.parametrize('value', [None, 0, 0.0, -1, 123.5, True, np.float32(2.0), np.int16(3), np.float64(F32_MAX)])
def test_values_that_pass(value):
    from amico_amd import prep
    assert prep.check_replace_bad_voxels(value) is value


def test_refusal_and_warning_carry_the_reference_sentences():
    """core.py:155, 158, 273, 276"""
    from amico_amd import prep
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        prep.refuse_or_warn(0, None, prep.BAD_RAW)           # nothing found: neither
        prep.refuse_or_warn(0, 0, prep.BAD_RAW)
    with pytest.raises(RuntimeError, match='Nan or Inf values in the raw signal. Try using the "replace_bad_voxels" or "b0_min_signal" parameters'):
        prep.refuse_or_warn(3, None, prep.BAD_RAW)
    with pytest.raises(RuntimeError, match='Nan or Inf values in the signal after the pre-processing. Try using'):
        prep.refuse_or_warn(1, None, prep.BAD_PREPROCESSED)
    with pytest.warns(UserWarning, match='Nan or Inf values in the raw signal. They will be replaced with: 0$'):
        prep.refuse_or_warn(3, 0, prep.BAD_RAW)
    with pytest.warns(UserWarning, match='Nan or Inf values in the signal after the pre-processing. They will be replaced with: 1.5'):
        prep.refuse_or_warn(3, 1.5, prep.BAD_PREPROCESSED)


def test_header_declares_the_entry_points():
    import os
    import re
    from amico_amd import _capi
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'amico_amd.h')).read()
    declared = set(re.findall(r'\b(amx_\w+)\s*\(', hdr))
    for n in ['amx_prep_sanitize', 'amx_prep_sanitize_device', 'amx_sanitize_device_f32', 'amx_sanitize_device', 'amx_sanitize',
              'amx_sanitize_last', 'amx_sanitize_previous']:
        assert n in declared and n in _capi.SYMBOLS, n
