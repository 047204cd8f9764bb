"""Gibbs unringing on the GPU (amx_prep_unring_device; include/amico_amd.h "(f0+++)") against the numpy oracle of
tests/unring_np.py, per pixel:

    |gpu - oracle| <= ulp32(|oracle|) + 4 C_U n_max eps64 max|slice|

C_U = 0.2314 is what the oracle and its restatement by matrices differ by on these very inputs (tests/test_unring.py); the margin is four
times that.  A pixel outside the bound passes only where it is within the bound of Ux_c + Uy_c' for oracle candidates c, c' whose window
variation lies within tau = 12 x the margin of the minimum (six differences of two values), and at most 1e-3 of a case's pixels may
(the restatement needed the clause for none).  Layouts, axis pairs, NaN / Inf slices, scaling by powers of two and repeated runs are held
to bit-identity."""
import functools

import numpy as np
import pytest

import unring_np as U
from amico_amd import synthetic as S
from test_unring import C_U

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def ctx():
    from amico_amd import get_context
    return get_context()


def make_plan(img):
    from amico_amd import _capi
    rank = np.arange(int(np.prod(img.shape[:3])), dtype=np.int32).reshape(img.shape[:3])
    return _capi.Prep(ctx(), img.shape, tuple(s // 4 for s in img.strides), rank, [[i] for i in range(img.shape[3])], np.zeros(0, dtype=np.int32))


def gpu(img, axes=(0, 1)):
    """-> (float32 image of img's shape and order, slices, passed_through); the output buffer has a sentinel tail that must stay and
    the image itself is only read"""
    import torch
    plan = make_plan(img)
    d = torch.from_numpy(np.array(plan._img_buffer(img))).to('cuda')
    out = torch.full((plan.extent + 64,), SENTINEL, dtype=torch.float32, device='cuda')
    slices, passed = plan.unring_device(d.data_ptr(), out.data_ptr(), axes)
    host = out.cpu().numpy()
    assert (host[plan.extent:] == SENTINEL).all()
    assert np.array_equal(d.cpu().numpy(), plan._img_buffer(img), equal_nan=True)
    plan.close()
    return np.lib.stride_tricks.as_strided(host[:plan.extent], shape=img.shape, strides=img.strides), slices, passed


@functools.lru_cache(maxsize=None)
def case(c):
    img = U.case_image(c)
    ref = U.unring64(img)
    img.setflags(write=False)
    ref.setflags(write=False)
    return img, ref


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('c', U.CASES)
def test_against_the_oracle(c):
    img, ref = case(c)
    got, slices, passed = gpu(img)
    assert slices == c[2] * c[3] and passed == 0
    worst, ties, out = U.compare(got, img, (0, 1), C_U, ref)
    print(f'{c}: worst |gpu - oracle| / bound {worst:.3f}; near-tie pixels {ties} of {got.size}; outside {out}')
    assert out == 0 and ties <= 1e-3 * got.size


@pytest.mark.parametrize('c', [(9, 17, 3, 5), (16, 33, 1, 5), (97, 64, 3, 1)])
def test_every_axis_pair_and_both_memory_orders_give_the_same_bits(c):
    img, _ = case(c)
    base, _, _ = gpu(img, (0, 1))
    f, slices, _ = gpu(np.asfortranarray(img), (0, 1))
    assert np.array_equal(bits(f), bits(base)) and slices == c[2] * c[3]
    # the same slices lying along other axes of the array: [a, c, b, v] unrung along (0, 2), [c, a, b, v] along (1, 2)
    for perm, axes in [((0, 2, 1, 3), (0, 2)), ((2, 0, 1, 3), (1, 2))]:
        moved = np.ascontiguousarray(img.transpose(perm))
        for arr in (moved, np.asfortranarray(moved)):
            got, slices, _ = gpu(arr, axes)
            assert slices == c[2] * c[3]
            assert np.array_equal(bits(got), bits(base.transpose(perm))), (perm, axes, arr.flags.c_contiguous)
    # the axes the other way round: the transposed slice's operator
    swapped, _, _ = gpu(np.ascontiguousarray(img.transpose(1, 0, 2, 3)), (1, 0))
    assert np.array_equal(bits(swapped), bits(base.transpose(1, 0, 2, 3)))


@pytest.mark.parametrize('c', [(8, 8, 3, 5), (15, 32, 3, 1), (31, 127, 1, 5)])
def test_one_nan_and_one_inf_slice(c):
    img, _ = case(c)
    clean, _, _ = gpu(img)
    bad = np.array(img)
    z1, s1, z2, s2 = c[2] - 1, c[3] - 1, 0, 0
    bad[c[0] - 1, c[1] - 1, z1, s1] = np.nan
    if (z1, s1) != (z2, s2):
        bad[0, 3, z2, s2] = -np.inf
    n_bad = 1 if (z1, s1) == (z2, s2) else 2
    for arr in (bad, np.asfortranarray(bad)):
        got, slices, passed = gpu(arr)
        assert slices == c[2] * c[3] and passed == n_bad
        keep = np.ones(c[2:], dtype=bool)
        keep[z1, s1] = keep[z2, s2] = False
        assert np.array_equal(bits(got[:, :, z1, s1]), bits(bad[:, :, z1, s1])) and np.array_equal(bits(got[:, :, z2, s2]), bits(bad[:, :, z2, s2]))
        assert np.array_equal(bits(got[:, :, keep]), bits(clean[:, :, keep]))


def test_a_zero_image_returns_zero():
    got, slices, passed = gpu(np.zeros((12, 19, 2, 3), dtype=np.float32))
    assert slices == 6 and passed == 0 and not bits(got).any()


@pytest.mark.parametrize('c', [(9, 17, 3, 5), (128, 31, 1, 1)])
def test_two_runs_are_bit_identical_and_powers_of_two_scale_exactly(c):
    img, _ = case(c)
    a, _, _ = gpu(img)
    b, _, _ = gpu(img)
    assert np.array_equal(bits(a), bits(b))
    for k in (-10, 14):
        f = np.float32(2.0 ** k)
        scaled, _, _ = gpu(img * f)
        assert np.array_equal(bits(scaled), bits(a * f)), k


def test_more_slices_than_a_chunk_holds():
    """256 x 200 pixels: eight slices more than a chunk holds take two chunks, and the bits of a slice do not depend on where in a chunk it lies"""
    from amico_amd import _capi
    n_a, n_b = 256, 200
    chunk = _capi.unring_route(n_a, n_b)['chunk']
    nS = chunk + 8
    one = U.noisy_image((n_a, n_b, 1, 3), seed=17)
    img = np.ascontiguousarray(one[:, :, :, np.arange(nS) % 3])
    got, slices, passed = gpu(img)
    assert slices == nS > chunk and passed == 0
    first, _, _ = gpu(np.ascontiguousarray(one))
    assert np.array_equal(bits(got), bits(first[:, :, :, np.arange(nS) % 3]))


def test_extents_outside_the_limit_and_other_bad_arguments():
    import torch
    from amico_amd import _capi, unring
    c = ctx()
    d = torch.zeros(257 * 8 * 7, dtype=torch.float32, device='cuda')
    out = torch.full((257 * 8 * 7,), SENTINEL, dtype=torch.float32, device='cuda')
    for shape, axes in [((7, 8, 2, 1), (0, 1)), ((8, 7, 2, 1), (0, 1)), ((257, 8, 1, 1), (0, 1)), ((7, 257, 8, 1), (1, 2)), ((8, 8, 7, 1), (2, 0))]:
        plan = make_plan(np.zeros(shape, dtype=np.float32))
        with pytest.raises(ValueError, match='8 to 256'):
            plan.unring_device(d.data_ptr(), out.data_ptr(), axes)
        plan.close()
        with pytest.raises(RuntimeError, match='8 to 256'):
            unring.unring(np.zeros(shape, dtype=np.float32), axes)
    plan = make_plan(np.zeros((8, 9, 2, 1), dtype=np.float32))
    for axes in [(0, 0), (0, 3), (-1, 1)]:
        with pytest.raises(ValueError, match='two different spatial axes'):
            plan.unring_device(d.data_ptr(), out.data_ptr(), axes)
    with pytest.raises(ValueError, match='null buffer'):
        plan.unring_device(d.data_ptr(), 0)
    with pytest.raises(ValueError, match='null buffer'):
        plan.unring_device(0, out.data_ptr())
    for bad_out in (d.data_ptr(), d.data_ptr() + 4 * (plan.extent - 1), d.data_ptr() - 4 * (plan.extent - 1)):
        with pytest.raises(ValueError, match='overlaps the image'):
            plan.unring_device(d.data_ptr(), bad_out)
    with pytest.raises(ValueError, match='not a plan'):
        c.check(_capi.lib().amx_prep_unring_device(c._h, None, d.data_ptr(), out.data_ptr(), 0, 1, None, None, None))
    plan.close()
    c.sync()
    assert (out.cpu().numpy() == SENTINEL).all()                  # a refused call writes nothing


def test_unring_numpy_in_numpy_out():
    from amico_amd import unring
    c = (16, 33, 1, 5)
    img, _ = case(c)
    base, _, _ = gpu(img)
    for arr in (np.array(img), np.asfortranarray(img)):
        res = unring.unring(arr)
        assert set(res) == {'image', 'slices', 'passed_through'} and res['slices'] == 5 and res['passed_through'] == 0
        assert res['image'].dtype == np.float32 and res['image'].shape == arr.shape and res['image'].strides == arr.strides
        assert np.array_equal(bits(res['image']), bits(base))
    vol = np.ascontiguousarray(img[:, :, 0, :])                   # three dimensions: [16, 33, 5], slices along the last axis
    for arr in (vol, np.asfortranarray(vol)):
        res = unring.unring(arr, axes=(0, 1))
        assert res['image'].shape == arr.shape and res['image'].strides == arr.strides and res['slices'] == 5
        assert np.array_equal(bits(res['image']), bits(base[:, :, 0, :]))
    res = unring.unring(vol.astype(np.float64)[::1], axes=[0, 1])  # any other dtype is copied to C-order float32
    assert np.array_equal(bits(res['image']), bits(base[:, :, 0, :]))
    with pytest.raises(ValueError, match='unring_axes'):
        unring.unring(vol, axes=(1, 1))


# ------------------------------------------------------------------ Evaluation
@pytest.fixture(scope='module')
def brain(htable500):
    """the fixture of tests/test_gpu_mppca_denoise.py: 16 x 16 x 8 voxels, one b0 volume and one shell of 30 directions at b = 1000, NODDI
    signals at SNR 20 on smoothly varying amplitudes around 1000, Fortran order, a mask of 0 / 1 / 2 that is mostly 1"""
    shape = (16, 16, 8)
    n = int(np.prod(shape))
    sch = S.make_scheme(1, ((1000.0, 30),), seed=2)
    ht = htable500['htable']
    K = S.noddi_kernels(sch, htable500['dirs'])
    y, _ = S.noddi_signals(n, K, ht, sch, seed=4, snr=1e6)
    g = np.stack(np.meshgrid(*[np.linspace(-1.0, 1.0, d) for d in shape], indexing='ij'), axis=-1)
    amp = (1000.0 * (1.0 + 0.2 * np.sin(2.0 * g[..., 0]) * np.cos(1.5 * g[..., 1]) + 0.1 * g[..., 2])).reshape(n, 1)
    rng = np.random.default_rng(6)
    clean = (y * amp).reshape(shape + (-1,))
    sg = 50.0
    img = np.abs(clean + sg * rng.standard_normal(clean.shape) + 1j * sg * rng.standard_normal(clean.shape)).astype(np.float32)
    mask = rng.choice(np.array([0, 1, 1, 1, 1, 1, 2], dtype=np.uint8), size=shape)
    return {'sch': sch, 'K': K, 'ht': ht, 'img': np.asfortranarray(img), 'mask': mask}


def run(brain, img=None, **config):
    import amico_amd
    ae = amico_amd.Evaluation()
    for key, value in config.items():
        ae.set_config(key.replace('DWI_SNR', 'DWI-SNR'), value)
    ae.set_data(brain['img'] if img is None else img, brain['sch'], brain['mask'])
    ae.set_model('NODDI')
    ae.set_kernels(brain['K'], brain['ht'])
    ae.fit()
    return ae


KEYS = ('MAPs', 'DIRs', 'DTI_outliers', 'DTI_MAPs', 'DTI_evals')
COMMON = dict(doDebiasSignal=True, DWI_SNR=20.0, DTI_fit_method='RESTORE', doSaveTensorMaps=True)


def test_evaluation_unring_is_the_fit_of_the_unringed_image(brain):
    """(A) doUnring with debias, RESTORE and tensor maps; (B) no key, fed the image of unring.unring: the same bits everywhere"""
    from amico_amd import unring
    a = run(brain, doUnring='Kellner', doSaveUnringedDWI=True, **COMMON)
    ref = unring.unring(brain['img'])
    assert a.get_config('unring_slices') == ref['slices'] == 8 * brain['sch'].nS and a.get_config('unring_passed_through') == ref['passed_through'] == 0
    got = a.RESULTS['DWI_unringed']
    assert got.dtype == np.float32 and got.shape == brain['img'].shape and np.array_equal(bits(got), bits(ref['image']))
    assert not np.array_equal(got, brain['img'])
    b = run(brain, img=ref['image'], **COMMON)
    for key in KEYS:
        assert np.array_equal(bits(a.RESULTS[key]), bits(b.RESULTS[key])), key
    assert np.array_equal(a.y, b.y)
    assert 'DWI_unringed' not in b.RESULTS and 'unring_slices' not in b.CONFIG and 'unring_passed_through' not in b.CONFIG
    plain = run(brain, **COMMON)
    assert not np.array_equal(plain.RESULTS['MAPs'], a.RESULTS['MAPs']) and set(a.RESULTS) - set(plain.RESULTS) == {'DWI_unringed'}
    # other axes: the slices along (2, 0)
    o = run(brain, doUnring=True, unring_axes=(0, 2), doSaveUnringedDWI=True)
    assert np.array_equal(bits(o.RESULTS['DWI_unringed']), bits(unring.unring(brain['img'], (0, 2))['image']))
    assert o.get_config('unring_slices') == 16 * brain['sch'].nS
    # the same Evaluation once more without the key: nothing lingers
    a.set_config('doUnring', False)
    a.set_data(brain['img'], brain['sch'], brain['mask'])
    a.fit()
    assert 'unring_slices' not in a.CONFIG and 'unring_passed_through' not in a.CONFIG and 'DWI_unringed' not in a.RESULTS
    assert np.array_equal(bits(a.RESULTS['MAPs']), bits(plain.RESULTS['MAPs']))


def test_evaluation_denoise_then_unring(brain):
    from amico_amd import noise, unring
    a = run(brain, doDenoise='MPPCA', doUnring=True, doSaveDenoisedDWI=True, doSaveUnringedDWI=True, doDebiasSignal=True)
    den = noise.denoise_mppca(brain['img'], brain['mask'], brain['sch'].b0_idx, patch=5)
    ref = unring.unring(den['image'])
    assert np.array_equal(bits(a.RESULTS['DWI_denoised']), bits(den['image']))
    assert np.array_equal(bits(a.RESULTS['DWI_unringed']), bits(ref['image']))
    assert a.get_config('DWI-SNR_estimated') == den['snr']        # the estimate is made before the unringing, on the image it always saw
    b = run(brain, img=ref['image'], doDebiasSignal=True, DWI_SNR=den['snr'])
    assert np.array_equal(bits(a.RESULTS['MAPs']), bits(b.RESULTS['MAPs'])) and np.array_equal(a.y, b.y)


def test_evaluation_extent_errors(brain):
    with pytest.raises(RuntimeError, match='doUnring.*8 to 256'):
        run(brain, img=brain['img'][:, :7], doUnring=True)
    with pytest.raises(ValueError, match='doUnring'):
        run(brain, doUnring='gibbs')
