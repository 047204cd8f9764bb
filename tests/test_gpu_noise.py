"""The noise estimate from the b0 repeats on the GPU (amx_noise_b0_*, amx_prep_noise_b0_device, amx_nanmedian_device; doEstimateNoise).

The per-voxel kernel and the median are exact statements, so every comparison here is bit for bit: the rows form against the numpy
restatement (tests/noise_np.py), the image form against the rows form on the gathered voxels, the median against np.partition on the
order-preserving keys and against np.nanmedian, and an Evaluation that estimates its noise against one that is handed the very numbers
the first one found."""
import numpy as np
import pytest

import noise_np as N
from amico_amd import synthetic as S

pytestmark = pytest.mark.gpu


def ctx():
    from amico_amd import get_context
    return get_context()


def same(a, b):
    """equal values with NaNs in the same places"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ------------------------------------------------------------------ rows form
def gpu_rows(rows, b0_idx, want=(True, True, True)):
    import torch
    from amico_amd import _capi
    c = ctx()
    d = torch.from_numpy(np.ascontiguousarray(rows)).to('cuda')
    n = rows.shape[0]
    out = [torch.full((n,), -7.0, dtype=torch.float64, device='cuda') if w else None for w in want]
    _capi.noise_b0_rows_device(c, d.data_ptr(), n, rows.shape[1], b0_idx, *[None if o is None else o.data_ptr() for o in out],
                               f32=rows.dtype == np.float32)
    c.sync()
    return [None if o is None else o.cpu().numpy() for o in out]


B0_LISTS = {2: [7, 2], 3: [9, 0, 4], 8: [10, 3, 8, 1, 6, 0, 5, 7], 9: [10, 2, 8, 0, 6, 4, 9, 1, 5],
            128: [int(i) for i in np.random.default_rng(128).permutation(130)[:128]]}


def make_rows(n, nS, b0_idx, dtype, amp, seed):
    """noisy rows around `amp`; from 63 rows on the first five are special: a NaN, a +Inf, no spread, a mean <= 0 (none of them
    eligible) and a NaN in a column that is no b0 (eligible: the kernel reads the b0 samples only)"""
    rng = np.random.default_rng(seed)
    rows = (amp * (1.0 + 0.05 * rng.standard_normal((n, nS)))).astype(dtype)
    bad = np.zeros(n, dtype=bool)
    if n >= 63:
        rows[0, b0_idx[1]] = np.nan
        rows[1, b0_idx[-1]] = np.inf
        rows[2, :] = dtype(amp)
        rows[3, b0_idx] = -rows[3, b0_idx]
        other = [j for j in range(nS) if j not in b0_idx]
        rows[4, other[0]] = np.nan
        bad[:4] = True
    return rows, bad


@pytest.mark.parametrize('k', [2, 3, 8, 9, 128])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_rows_form_bit_for_bit(dtype, k):
    b0_idx = B0_LISTS[k]
    nS = 130 if k == 128 else 11
    assert sorted(b0_idx) != b0_idx and len(set(b0_idx)) == k and sorted(b0_idx) != list(range(min(b0_idx), min(b0_idx) + k))
    for n in (1, 63, 64, 65, 1000):
        for amp in (2.0 ** -10, 2.0 ** 14):
            rows, bad = make_rows(n, nS, b0_idx, dtype, amp, seed=1000 * k + n)
            want = N.per_voxel(rows, b0_idx)
            got = gpu_rows(rows, b0_idx)
            for name, g, w in zip(('mean', 'sd', 'ratio'), got, want):
                assert same(g, w), (name, n, amp)
                assert np.array_equal(np.isnan(g), bad), (name, n, amp)
            # the NaN of an ineligible voxel is the same in all three outputs; a single output may be asked for alone
            only = gpu_rows(rows, b0_idx, want=(False, False, True))
            assert only[0] is None and only[1] is None and same(only[2], want[2])


def test_rows_form_arguments():
    import torch
    from amico_amd import _capi
    c = ctx()
    rows = np.ones((4, 11), dtype=np.float32)
    d = torch.from_numpy(rows).to('cuda')
    o = torch.full((4,), -7.0, dtype=torch.float64, device='cuda')
    for b0, sentence in (([3], 'at least 2'), (list(range(11)) * 12, 'more than 128'), ([0, 11], 'out of range'), ([-1, 2], 'out of range')):
        with pytest.raises(ValueError, match=sentence):
            _capi.noise_b0_rows_device(c, d.data_ptr(), 4, 11, b0, o.data_ptr(), None, None, f32=True)
    with pytest.raises(ValueError, match='at least one'):
        _capi.noise_b0_rows_device(c, d.data_ptr(), 4, 11, [0, 1], None, None, None, f32=True)
    _capi.noise_b0_rows_device(c, 0, 0, 11, [0, 1], o.data_ptr(), None, None, f32=True)          # n == 0: a no-op
    c.sync()
    assert (o.cpu().numpy() == -7.0).all()


def test_estimate_from_rows_is_the_restatement():
    from amico_amd import noise
    from test_noise import rician_rows
    for k, snr in ((2, 10.0), (6, 30.0)):
        rows, b0_idx, sg = rician_rows(4001, k, snr)
        rows[5, b0_idx] = 3.0                                  # one voxel without spread
        got, want = noise.estimate_from_rows(rows, b0_idx), N.estimate(rows, b0_idx)
        assert got['voxels'] == want['voxels'] == 4000
        assert got['snr'] == want['snr'] and got['sigma'] == want['sigma']
        assert same(got['mean'], want['mean']) and same(got['sd'], want['sd'])
    empty = noise.estimate_from_rows(np.ones((7, 5)), [0, 1, 2])
    assert empty['voxels'] == 0 and np.isnan(empty['snr']) and np.isnan(empty['sigma']) and np.isnan(empty['mean']).all()


# ------------------------------------------------------------------ image form
def scheme_with_b0_at(nS, b0_at):
    rng = np.random.default_rng(3)
    g = rng.standard_normal((nS, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return S.SimpleScheme(np.column_stack([g, np.where(np.isin(np.arange(nS), b0_at), 0.0, 1000.0)]))


@pytest.mark.parametrize('layout', ['C', 'F', 'strided'])
def test_image_form_against_rows_form(layout):
    import torch
    from amico_amd import prep
    shape, nS = (5, 7, 9), 11
    sch = scheme_with_b0_at(nS, [0, 3, 4, 9])
    assert list(sch.b0_idx) == [0, 3, 4, 9]
    rng = np.random.default_rng(17)
    values = (900.0 * (1.0 + 0.05 * rng.standard_normal(shape + (nS,)))).astype(np.float32)
    values[1, 2, 3, 3] = np.nan                               # an ineligible voxel inside the mask
    values[2, 2, 2, :] = 5.0
    mask = rng.choice(np.array([0, 1, 1, 2], dtype=np.uint8), size=shape)
    mask[1, 2, 3] = mask[2, 2, 2] = 1
    if layout == 'strided':
        parent = np.full((5, 7, 18, 13), np.nan, dtype=np.float32)      # NaN between the view's elements: reading one would show
        img = parent[:, :, ::2, 1:12]
        img[...] = values
    else:
        img = np.asarray(values, order=layout)
    sp = prep.SignalPreparation(sch, img, mask, do_normalize=False)
    assert sp.n_vox == int((mask == 1).sum())
    flat = np.array(sp._plan._img_buffer(img))
    d = torch.from_numpy(flat).to('cuda')
    out = torch.full((3, sp.n_vox), -7.0, dtype=torch.float64, device='cuda')
    sp._plan.noise_b0_device(d.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    sp.ctx.sync()
    got = out.cpu().numpy()
    want = gpu_rows(np.ascontiguousarray(values[mask == 1]), sch.b0_idx)          # the fit's selection and order: mask == 1, C order
    for g, w in zip(got, want):
        assert same(g, w)
    assert np.isnan(got).any(axis=0).sum() == 2 and same(got[0], N.per_voxel(values[mask == 1], sch.b0_idx)[0])
    # the image, and with a strided view whatever lies between its elements, is as it was
    assert np.array_equal(d.cpu().numpy().view(np.uint32), flat.view(np.uint32))


# ------------------------------------------------------------------ the exact median
def gpu_median(v, stream=None, d=None):
    import torch
    from amico_amd import _capi
    c = ctx()
    if d is None:
        d = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to('cuda')
        torch.cuda.synchronize()
    out = torch.full((3,), -7.0, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    _capi.nanmedian_device(c, d.data_ptr(), d.numel(), out.data_ptr(), out.data_ptr() + 16, stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    return host[0], host[1], int(host[2:3].view(np.int64)[0])


def from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def median_case(case, n, rng):
    if case == 'low_byte':                # equal but for the lowest byte: every digit pass decides, the last one among many
        return from_bits(np.uint64(0x3FF0000000000000) | rng.integers(0, 256, size=n, dtype=np.uint64))
    if case == 'top_byte':                # equal but for the top byte (sign and high exponent bits; no NaN or Inf among them)
        return from_bits((rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x0012345678ABCDEF))
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)
    if case == 'duplicates':
        v[rng.random(n) < 0.9] = 0.7321
    elif case == 'all_equal':
        v[:] = -3.25
    elif case == 'inf':
        v[rng.random(n) < 0.3] = np.inf
        v[rng.random(n) < 0.3] = -np.inf
    elif case == 'mostly_inf':
        v[rng.random(n) < 0.8] = np.inf
    elif case == 'nan50':
        v[rng.random(n) < 0.5] = np.nan
    elif case == 'nan100':
        v[:] = np.nan
    elif case == 'zeros':                 # the middle falls among zeros of both signs
        v = np.where(rng.random(n) < 0.5, -0.0, 0.0)
        v[rng.random(n) < 0.1] = -1.0
        v[rng.random(n) < 0.1] = 1.0
    else:
        assert case == 'mixed_sign'
    return v


MEDIAN_SIZES = (1, 2, 3, 255, 256, 257, 4097, 100003)


@pytest.mark.parametrize('case', ['low_byte', 'top_byte', 'duplicates', 'all_equal', 'mixed_sign', 'inf', 'mostly_inf', 'nan50', 'nan100', 'zeros'])
def test_median_is_exact(case):
    rng = np.random.default_rng(sum(map(ord, case)))
    for n in MEDIAN_SIZES:
        v = median_case(case, n, rng)
        lo, hi, c = gpu_median(v)
        wlo, whi, wc = N.middles(v)
        assert c == wc == int((~np.isnan(v)).sum()), (case, n)
        # both middle values by bit pattern (-0.0 is not +0.0 here)
        assert np.array_equal(np.array([lo, hi]).view(np.uint64), np.array([wlo, whi]).view(np.uint64)), (case, n, lo, hi, wlo, whi)
        if c:
            with np.errstate(invalid='ignore', over='ignore'):
                assert same((lo + hi) / 2.0, np.nanmedian(v)), (case, n)           # (+Inf and -Inf in the middle: NaN in both)


def test_median_empty_input():
    import torch
    from amico_amd import _capi
    c = ctx()
    out = torch.full((3,), -7.0, dtype=torch.float64, device='cuda')
    _capi.nanmedian_device(c, 0, 0, out.data_ptr(), out.data_ptr() + 16)
    c.sync()
    host = out.cpu().numpy()
    assert np.isnan(host[0]) and np.isnan(host[1]) and host[2:3].view(np.int64)[0] == 0
    with pytest.raises(ValueError):
        _capi.nanmedian_device(c, 0, 5, out.data_ptr(), out.data_ptr() + 16)
    with pytest.raises(ValueError):
        _capi.nanmedian_device(c, out.data_ptr(), 3, 0, out.data_ptr() + 16)


def test_median_streams_and_workspace_reuse():
    """the same input on two streams, and again after a larger call has used the workspace: the same bits"""
    import torch
    rng = np.random.default_rng(5)
    v = rng.standard_normal(4097)
    v[::7] = np.nan
    d = torch.from_numpy(v).to('cuda')
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = gpu_median(v, stream=s1.cuda_stream, d=d)
    second = gpu_median(v, stream=s2.cuda_stream, d=d)
    big = rng.standard_normal(100003)
    assert gpu_median(big)[2] == 100003
    third = gpu_median(v, d=d)
    want = N.middles(v)
    for got in (first, second, third):
        assert np.array_equal(np.array(got[:2]).view(np.uint64), np.array(want[:2]).view(np.uint64)) and got[2] == want[2]


# ------------------------------------------------------------------ Evaluation
@pytest.fixture(scope='module')
def brain(htable500):
    """12 x 12 x 10 voxels, 6 b0 volumes and one shell of 30 directions at b = 1000 (a tensor fits it), NODDI signals at SNR 20 on
    amplitudes of 700 .. 1300, a mask of 0 / 1 / 2.  The NODDI kernels are made for this scheme on the golden table's 500 directions
    (the golden NODDI fixture's own kernels belong to its 99-volume scheme and hold a handful of orientations)"""
    shape = (12, 12, 10)
    n = int(np.prod(shape))
    sch = S.make_scheme(6, ((1000.0, 30),), seed=2)
    ht = htable500['htable']
    K = S.noddi_kernels(sch, htable500['dirs'])
    y, _ = S.noddi_signals(n, K, ht, sch, seed=4, snr=1e6)          # (clean: the noise is added below, on the amplitudes)
    rng = np.random.default_rng(6)
    amp = rng.uniform(700.0, 1300.0, size=(n, 1))
    clean = (y * amp).reshape(shape + (-1,))
    sg = (amp / 20.0).reshape(shape + (1,))
    img = np.abs(clean + sg * rng.standard_normal(clean.shape) + 1j * sg * rng.standard_normal(clean.shape)).astype(np.float32)
    mask = rng.choice(np.array([0, 1, 1, 1, 2], dtype=np.uint8), size=shape)
    return {'sch': sch, 'K': K, 'ht': ht, 'img': np.asfortranarray(img), 'mask': mask}


def run(brain, img=None, scaling=None, mask=None, **config):
    import amico_amd
    ae = amico_amd.Evaluation()
    for key, value in config.items():
        ae.set_config(key.replace('DWI_SNR', 'DWI-SNR'), value)
    ae.set_data(brain['img'] if img is None else img, brain['sch'], brain['mask'] if mask is None else mask, scaling=scaling)
    ae.set_model('NODDI')
    ae.set_kernels(brain['K'], brain['ht'])
    ae.fit()
    return ae


def assert_same_results(a, b, keys):
    for key in keys:
        assert np.array_equal(a.RESULTS[key].view(np.uint32), b.RESULTS[key].view(np.uint32)), key
    assert tuple(a.get_config('dti_robust')) == tuple(b.get_config('dti_robust'))
    assert np.array_equal(a.y, b.y)


RESTORE_KEYS = ('MAPs', 'DIRs', 'DTI_outliers', 'DTI_MAPs', 'DTI_evals')


def test_evaluation_estimate_equals_the_numbers_handed_in(brain):
    """(A) the key, debias and RESTORE with no SNR and no sigma; (B) no key, DWI-SNR = what (A) found: the same bits everywhere"""
    a = run(brain, doEstimateNoise=True, doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True)
    snr, sigma, c = a.get_config('DWI-SNR_estimated'), a.get_config('noise_sigma_estimated'), a.get_config('noise_voxels')
    print(f'estimated SNR {snr:.3f} (made at 20), sigma {sigma:.3f} (amplitudes 700 .. 1300 at SNR 20: 35 .. 65), {c} voxels')
    # a sanity bound, not the accuracy test (tests/test_noise.py): sd of nu = 5 scatters by 1 / sqrt(2 nu) = 32 %, its median over c
    # voxels by 1.25 * 32 % / sqrt(c) = 1.3 % at c = 900, the Rician bias at SNR 20 is below 1 %: 10 % is seven such deviations.
    # Every voxel's sigma lies in 35 .. 65 by construction
    assert c == int((brain['mask'] == 1).sum()) and abs(snr / 20.0 - 1.0) < 0.10 and 35.0 < sigma < 65.0
    assert a.get_config('DWI-SNR') is None and a.get_config('DTI_sigma') is None
    b = run(brain, doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True, DWI_SNR=snr)
    assert 'NOISE_MAPs' not in b.RESULTS and b.get_config('DWI-SNR_estimated') is None
    assert_same_results(a, b, RESTORE_KEYS)
    print('RESTORE counters', tuple(a.get_config('dti_robust')), 'samples left out', int(a.RESULTS['DTI_outliers'].sum()))


def test_evaluation_estimate_without_normalisation(brain):
    """the same pair with doNormalizeSignal off: `y` is in image units and (B) is handed DTI_sigma = noise_sigma_estimated"""
    a = run(brain, doEstimateNoise=True, doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True, doNormalizeSignal=False)
    snr, sigma = a.get_config('DWI-SNR_estimated'), a.get_config('noise_sigma_estimated')
    b = run(brain, doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True, doNormalizeSignal=False, DWI_SNR=snr, DTI_sigma=sigma)
    assert_same_results(a, b, RESTORE_KEYS)
    # ... and DWI-SNR alone gives a robust fit no sigma there, with or without the estimate's help for the debias
    with pytest.raises(NotImplementedError):
        run(brain, doDebiasSignal=True, DTI_fit_method='RESTORE', doNormalizeSignal=False, DWI_SNR=snr)


def test_explicit_snr_wins_and_the_estimate_is_still_reported(brain):
    off = run(brain, doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True, DWI_SNR=17.0)
    on = run(brain, doEstimateNoise=True, doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True, DWI_SNR=17.0)
    assert_same_results(on, off, RESTORE_KEYS)
    est = run(brain, doEstimateNoise=True)
    assert on.get_config('DWI-SNR_estimated') == est.get_config('DWI-SNR_estimated') != 17.0
    assert on.get_config('noise_sigma_estimated') == est.get_config('noise_sigma_estimated')
    assert on.get_config('DWI-SNR') == 17.0
    # the key alone changes nothing of a plain fit
    plain = run(brain)
    assert np.array_equal(est.RESULTS['MAPs'], plain.RESULTS['MAPs']) and np.array_equal(est.RESULTS['DIRs'], plain.RESULTS['DIRs'])
    assert set(est.RESULTS) - set(plain.RESULTS) == {'NOISE_MAPs'}


def test_noise_maps_and_estimates_are_the_restatement(brain):
    ae = run(brain, doEstimateNoise=True)
    sel = brain['mask'] == 1
    want = N.estimate(brain['img'][sel], brain['sch'].b0_idx)
    assert ae.get_config('DWI-SNR_estimated') == want['snr'] and ae.get_config('noise_sigma_estimated') == want['sigma']
    assert ae.get_config('noise_voxels') == want['voxels']
    vol = np.zeros(sel.shape + (2,), dtype=np.float32)
    vol[sel, 0] = np.nan_to_num(want['mean'], nan=0.0).astype(np.float32)
    vol[sel, 1] = np.nan_to_num(want['sd'], nan=0.0).astype(np.float32)
    got = ae.RESULTS['NOISE_MAPs']
    assert got.dtype == np.float32 and got.shape == vol.shape and np.array_equal(got, vol)
    # a voxel without spread inside the mask: zero in both maps, one voxel fewer
    img = brain['img'].copy(order='F')
    where = tuple(np.argwhere(sel)[10])
    img[where][brain['sch'].b0_idx] = 500.0
    ae2 = run(brain, img=img, doEstimateNoise=True)
    assert ae2.get_config('noise_voxels') == want['voxels'] - 1 and not ae2.RESULTS['NOISE_MAPs'][where].any()


def test_stored_dtype_image_gives_the_same_estimate(brain):
    """int16 with a scaling goes through the ingest kernel; its float32 equivalent through the plain upload: one estimate"""
    from amico_amd import prep
    raw = np.asfortranarray(np.round(brain['img'] * 2.0).astype(np.int16))
    scaling = (0.5, 3.0)
    img32 = np.asfortranarray(prep.to_float32(raw, scaling))
    a = run(brain, img=raw, scaling=scaling, doEstimateNoise=True, doDebiasSignal=True)
    b = run(brain, img=img32, doEstimateNoise=True, doDebiasSignal=True)
    assert a._raw is not None and b._raw is None
    for key in ('DWI-SNR_estimated', 'noise_sigma_estimated', 'noise_voxels'):
        assert a.get_config(key) == b.get_config(key), key
    assert np.array_equal(a.RESULTS['MAPs'], b.RESULTS['MAPs']) and np.array_equal(a.RESULTS['NOISE_MAPs'], b.RESULTS['NOISE_MAPs'])


def test_no_eligible_voxel_is_an_error(brain):
    img = brain['img'].copy(order='F')
    img[..., brain['sch'].b0_idx] = 800.0                       # every b0 repeat equal: no spread anywhere
    with pytest.raises(RuntimeError, match='doEstimateNoise'):
        run(brain, img=img, doEstimateNoise=True)
