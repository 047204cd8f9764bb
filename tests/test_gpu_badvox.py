"""replace_bad_voxels on the GPU (amx_sanitize*, amx_prep_sanitize*; core.py:152-158 and 270-276).

The model is tests/badvox_np.py (the reference's isnan / isinf test and its nan_to_num call); counts are compared exactly and buffers
bit for bit through integer views, so -0.0, denormals and NaN payloads are seen.  No test hands a non-finite value to a solver kernel:
the refusal tests rely on Evaluation.fit() reading each count before it enqueues anything behind the scan."""
import warnings

import numpy as np
import pytest

import badvox_np as B
from amico_amd import synthetic as S

pytestmark = pytest.mark.gpu
RAW_WARNING = 'Nan or Inf values in the raw signal. They will be replaced with'
NAN32, NAN64_HI = 0x7fc00000, 0x7ff80000


def ctx():
    from amico_amd import get_context
    return get_context()


def plant(a, where, rng):
    a[where] = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=len(where)).astype(a.dtype)


# ---------------------------------------------------------------- 1. flat scan

@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_flat_scan(dtype):
    """2^24 + 13 elements starting 4 bytes into a tensor, 1 000 planted NaN / +Inf / -Inf: the first element, the last one and the
    unaligned tail among them; the words either side of the buffer hold NaN patterns that must be neither counted nor touched"""
    import torch
    from amico_amd import _capi
    c = ctx()
    n = 2 ** 24 + 13
    rng = np.random.default_rng(5)
    data = rng.standard_normal(n).astype(dtype)
    data[rng.choice(n, 4000, replace=False)] = np.array([-0.0, 1e-45, -1e-45, np.finfo(np.float32).max], dtype=dtype).repeat(1000)
    where = np.concatenate([[0, n - 3, n - 2, n - 1], 1 + rng.choice(n - 4, 996, replace=False)])      # seeded random positions + the ends
    assert len(np.unique(where)) == 1000
    plant(data, where, rng)
    assert B.count(data) == 1000
    f32 = dtype == np.float32
    wpe = 1 if f32 else 2                                       # 32-bit words per element
    words = np.empty(n * wpe + 2, dtype=np.int32)
    words[0] = NAN32
    words[-1] = NAN32 if f32 else NAN64_HI                      # (would be the high word of a float64 NaN)
    words[1:-1] = data.view(np.int32)
    for r in (None, 0.0, 123.5):
        d = torch.from_numpy(words).to('cuda')
        _capi.sanitize_device(c, d.data_ptr() + 4, n, r, f32=f32)
        assert c.sanitize_last() == 1000, r
        back = d.cpu().numpy()
        assert back[0] == words[0] and back[-1] == words[-1]
        want = data if r is None else B.replace(data, r)
        assert np.array_equal(back[1:-1], want.view(np.int32)), r
    # a second pass over a cleaned buffer finds nothing and the count of the call before it is still there
    _capi.sanitize_device(c, d.data_ptr() + 4, n, None, f32=f32)
    assert c.sanitize_last() == 0 and c.sanitize_previous() == 1000
    with pytest.raises(ValueError, match='finite'):
        _capi.sanitize_device(c, d.data_ptr() + 4, n, float('inf'), f32=f32)
    _capi.sanitize_device(c, d.data_ptr() + 4, 0, 0.0, f32=f32)
    assert c.sanitize_last() == 0


@pytest.mark.parametrize('n', [1, 2, 3, 5, 7, 64, 1027])
def test_flat_scan_short_buffers(n):
    """lengths below and around one vector, every start alignment: head and tail handling"""
    import torch
    from amico_amd import _capi
    c = ctx()
    rng = np.random.default_rng(n)
    for off in range(4):
        data = rng.standard_normal(n).astype(np.float32)
        where = np.unique(np.concatenate([[0, n - 1], rng.choice(n, max(1, n // 3))]))
        plant(data, where, rng)
        words = np.full(n + off + 4, NAN32, dtype=np.int32)
        words[off:off + n] = data.view(np.int32)
        d = torch.from_numpy(words).to('cuda')
        _capi.sanitize_device(c, d.data_ptr() + 4 * off, n, -2.0)
        assert c.sanitize_last() == len(where)
        want = words.copy()
        want[off:off + n] = B.replace(data, -2.0).view(np.int32)
        assert np.array_equal(d.cpu().numpy(), want), (n, off)


# ---------------------------------------------------------------- 2. image form

def scheme33():
    b = np.where(np.arange(33) % 11 == 0, 0.0, 1000.0)
    return S.SimpleScheme(np.column_stack([np.tile([1.0, 0.0, 0.0], (33, 1)), b]))


def image_case(view, base, r):
    """`view`: the image (a view of `base` or `base` itself).  -> nothing; asserts count and contents of the device and host forms"""
    import torch
    from amico_amd import prep
    mask = np.random.default_rng(2).choice(np.array([0, 1, 1, 2], dtype=np.uint8), size=view.shape[:3])
    sp = prep.SignalPreparation(scheme33(), view, mask, do_normalize=False)
    want_count = B.count(view)
    assert want_count > 0
    flat = np.array(sp._plan._img_buffer(view))                  # the extent, gaps included
    for rr in (None, r):
        d = torch.from_numpy(flat).to('cuda')
        sp._plan.sanitize_device(d.data_ptr(), rr)
        assert sp.ctx.sanitize_last() == want_count
        want = np.array(flat)
        if rr is not None:
            np.lib.stride_tricks.as_strided(want, shape=view.shape, strides=view.strides)[...] = B.replace(view, rr)
        assert np.array_equal(B.bits(d.cpu().numpy()), B.bits(want))
    # host form, in place on a private copy of the extent
    host = np.array(flat)
    himg = np.lib.stride_tricks.as_strided(host, shape=view.shape, strides=view.strides)
    assert sp._plan.sanitize(himg, r) == want_count
    assert np.array_equal(B.bits(host), B.bits(want))
    assert sp._plan.sanitize(himg, None) == 0
    return want_count


def make_image(shape, order, seed, frac=0.01):
    rng = np.random.default_rng(seed)
    img = np.asarray(rng.uniform(0.0, 1000.0, size=shape).astype(np.float32), order=order)
    flat = img.reshape(-1, order=order)
    assert np.shares_memory(flat, img)
    flat[rng.choice(flat.size, 100, replace=False)] = np.float32(-0.0)
    plant(flat, rng.choice(flat.size, int(frac * flat.size), replace=False), rng)
    return img


@pytest.mark.parametrize('order', ['C', 'F'])
def test_image_form_dense(order):
    img = make_image((24, 20, 16, 33), order, seed=7)
    assert image_case(img, img, 0.0) == int(0.01 * img.size)
    image_case(img, img, 123.5)


def test_image_form_views_with_gaps():
    """every second volume of a larger image, and a slab of a larger buffer: NaNs sit in the gaps too, and they are neither counted
    nor written"""
    big = make_image((24, 20, 16, 66), 'C', seed=8, frac=0.02)
    view = big[:, :, :, ::2]
    assert view.shape == (24, 20, 16, 33) and 0 < B.count(view) < B.count(big)
    image_case(view, big, 0.0)
    big2 = make_image((28, 20, 17, 33), 'C', seed=9, frac=0.02)
    slab = big2[2:-2, :, 1:]
    assert slab.shape == (24, 20, 16, 33) and B.count(big2[2:-2, :, 0]) > 0
    image_case(slab, big2, 7.25)
    big3 = make_image((24, 21, 16, 33), 'F', seed=10, frac=0.02)
    image_case(big3[:, 1:], big3, 0.0)


# ---------------------------------------------------------------- 3-6. Evaluation

SHAPE = (10, 8, 6)


@pytest.fixture(scope='module')
def noddi(htable500):
    sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, htable500['dirs'])
    y, _ = S.noddi_signals(int(np.prod(SHAPE)), K, htable500['htable'], sch, seed=6)
    img = np.asfortranarray((y.reshape(SHAPE + (-1,)) * 800.0).astype(np.float32))
    mask = np.random.default_rng(4).choice(np.array([0, 1, 1, 1, 2], dtype=np.uint8), size=SHAPE)
    return dict(sch=sch, K=K, ht=htable500['htable'], img=img, mask=mask)


def evaluation(f, img, mask=None, replace=None, debias=None):
    import amico_amd
    ae = amico_amd.Evaluation()
    if debias is not None:
        ae.set_config('doDebiasSignal', True)
        ae.set_config('DWI-SNR', debias)
    ae.set_data(img, f['sch'], f['mask'] if mask is None else mask, replace_bad_voxels=replace)
    ae.set_model('NODDI')
    ae.set_kernels(f['K'], f['ht'])
    return ae


def same_results(a, b):
    assert set(a.RESULTS) == set(b.RESULTS)
    for k in a.RESULTS:
        assert np.array_equal(B.bits(a.RESULTS[k]), B.bits(b.RESULTS[k])), k


def bad_image(f, seed=12):
    """NaN and +-Inf in about 1 % of the samples, inside and outside the mask"""
    img = np.array(f['img'], order='F')
    rng = np.random.default_rng(seed)
    hit = rng.random(img.shape) < 0.01
    img[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size=int(hit.sum()))
    assert B.bad(img)[f['mask'] == 1].any() and B.bad(img)[f['mask'] == 0].any()
    return img


def test_evaluation_finite_image_is_untouched(noddi):
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        a = evaluation(noddi, noddi['img'], replace=None)
        a.fit()
        b = evaluation(noddi, noddi['img'], replace=0)
        b.fit()
    same_results(a, b)
    assert 'MAPs' in a.RESULTS and 'DIRs' in a.RESULTS
    for ae in (a, b):
        assert ae.get_config('bad_samples_raw') == 0 and ae.get_config('bad_samples_preprocessed') == 0
    assert a.get_config('replace_bad_voxels') is None and b.get_config('replace_bad_voxels') == 0


@pytest.mark.parametrize('debias', [None, 25.0])
def test_evaluation_replaces_bad_samples(noddi, debias):
    """the fit of the image with its bad samples replaced in HBM IS the fit of the image numpy cleaned -- with doDebiasSignal as well,
    which shows that the replacement comes before the debias"""
    img = bad_image(noddi)
    ae = evaluation(noddi, img, replace=0.0, debias=debias)
    with pytest.warns(UserWarning, match=RAW_WARNING):
        ae.fit()
    ref = evaluation(noddi, B.replace(img, 0.0), replace=None, debias=debias)
    ref.fit()
    same_results(ae, ref)
    assert ae.get_config('bad_samples_raw') == B.count(img) > 0 and ref.get_config('bad_samples_raw') == 0
    assert np.array_equal(B.bits(ae.niiDWI_img), B.bits(img))          # the host image keeps the planted values
    assert np.array_equal(ae.y, ref.y) and np.isfinite(ae.y).all()


def test_evaluation_refuses_without_a_value(noddi):
    img = np.array(noddi['img'], order='F')
    out = np.argwhere(noddi['mask'] == 0)[0]
    img[out[0], out[1], out[2], 17] = np.nan                             # a single NaN, outside the mask
    ae = evaluation(noddi, img)
    with pytest.raises(RuntimeError, match='Nan or Inf values in the raw signal'):
        ae.fit()
    assert ae.RESULTS is None and ae._dev is None and ae.get_config('bad_samples_raw') == 1
    # the same process, the same object, a clean image: fits
    ae.set_data(noddi['img'], noddi['sch'], noddi['mask'])
    ae.fit()
    ok = evaluation(noddi, noddi['img'])
    ok.fit()
    same_results(ae, ok)


def test_second_check_after_the_preprocessing(noddi):
    """a finite raw image whose normalisation overflows float32 in one masked voxel: b0 samples 2e-38 (a normal float32), DWI samples
    100 -> 100 * float32(1 / 2e-38) = +Inf"""
    sch = noddi['sch']
    img = np.array(noddi['img'], order='F')
    v = tuple(np.argwhere(noddi['mask'] == 1)[5])
    img[v][sch.b0_idx] = np.float32(2e-38)
    img[v][sch.dwi_idx] = np.float32(100.0)
    assert np.isfinite(img).all() and img[v][sch.b0_idx[0]] == np.float32(2e-38)
    ae = evaluation(noddi, img)
    with pytest.raises(RuntimeError, match='after the pre-processing'):
        ae.fit()
    assert ae.get_config('bad_samples_raw') == 0 and ae.get_config('bad_samples_preprocessed') == len(sch.dwi_idx)
    assert ae.RESULTS is None
    ae = evaluation(noddi, img, replace=0)
    with pytest.warns(UserWarning, match='Nan or Inf values in the signal after the pre-processing. They will be replaced with: 0'):
        ae.fit()
    assert ae.get_config('bad_samples_raw') == 0 and ae.get_config('bad_samples_preprocessed') == len(sch.dwi_idx)
    row = ae.y[int((noddi['mask'] == 1).ravel()[:np.ravel_multi_index(v, SHAPE)].sum())]
    assert np.array_equal(row[sch.b0_idx], np.ones(len(sch.b0_idx))) and not row[sch.dwi_idx].any()
    mask2 = noddi['mask'].copy()
    mask2[v] = 0
    ref = evaluation(noddi, img, mask=mask2)
    ref.fit()
    others = mask2 == 1
    for k in ('MAPs', 'DIRs'):
        assert np.array_equal(B.bits(ae.RESULTS[k][others]), B.bits(ref.RESULTS[k][others])), k


# ---------------------------------------------------------------- 7. the device-resident chain, 8. the host-array preparation

@pytest.mark.parametrize('fused', [True, False])
def test_volume_pipeline(noddi, fused):
    import torch
    from amico_amd import pipeline
    img = bad_image(noddi)
    clean = B.replace(img, 0.0)
    args = (noddi['sch'], img, noddi['mask'], noddi['K'], noddi['ht'])

    def dev(a):
        return torch.from_numpy(np.lib.stride_tricks.as_strided(a, shape=(a.size,), strides=(4,)).copy()).to('cuda:0')
    pl = pipeline.NoddiVolumePipeline(*args, fused=fused, replace_bad_voxels=0.0)
    d_img = dev(img)
    maps, dirs = (t.cpu().numpy() for t in pl.run(d_img))
    assert pl.bad_samples == B.count(img) and pl.bad_samples_preprocessed == 0
    assert np.array_equal(B.bits(d_img.cpu().numpy()), B.bits(clean.reshape(-1, order='F')))
    plain = pipeline.NoddiVolumePipeline(*args, fused=fused)
    maps0, dirs0 = (t.cpu().numpy() for t in plain.run(dev(clean)))
    assert plain.bad_samples is None
    assert np.array_equal(B.bits(maps), B.bits(maps0)) and np.array_equal(B.bits(dirs), B.bits(dirs0))
    if not fused:
        # None on a clean image: the chain as it was -- gather, tensor fit, NODDI fit and scatter are the calls Evaluation.fit makes
        ae = evaluation(noddi, clean)
        ae.fit()
        assert np.array_equal(maps0, ae.RESULTS['MAPs']) and np.array_equal(dirs0, ae.RESULTS['DIRs'])


def test_signal_preparation_host_arrays(noddi):
    from amico_amd import prep
    img = bad_image(noddi)
    sp = prep.SignalPreparation(noddi['sch'], img, noddi['mask'], replace_bad_voxels=0)
    with pytest.warns(UserWarning, match=RAW_WARNING):
        y, mb0 = sp.gather(img)
    assert sp.bad_samples_raw == B.count(img) and sp.bad_samples_preprocessed == 0
    assert B.count(img) > 0                                            # gather worked on a copy
    sp0 = prep.SignalPreparation(noddi['sch'], img, noddi['mask'])
    y0, mb00 = sp0.gather(B.replace(img, 0.0))
    assert np.array_equal(y, y0) and np.array_equal(mb0, mb00) and sp0.bad_samples_raw is None
    # the float64 host form on its own
    from amico_amd import _capi
    a = np.array(y0)
    a[3, 5], a[0, 0], a[-1, -1] = np.nan, np.inf, -np.inf
    b = a.copy()
    assert _capi.sanitize(sp.ctx, b, None) == 3 and np.array_equal(B.bits(a), B.bits(b))
    assert _capi.sanitize(sp.ctx, b, 0.5) == 3 and np.array_equal(B.bits(b), B.bits(B.replace(a, 0.5)))
