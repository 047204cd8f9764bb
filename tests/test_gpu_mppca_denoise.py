"""The Marchenko-Pastur denoiser on the GPU (k_mppca_denoise, amx_prep_noise_mppca_denoise_device; doDenoise = 'MPPCA') against
the float64 SVD reference of tests/mppca_denoise_np.py, on the shapes of tests/test_gpu_mppca.py (the branches are the same) and on
images of high rank.

Bound.  A denoised row may differ from the reference's by  C_DEN eps (q + r) (lambda_max / gap) |x_c|  (tests/test_mppca_denoise.py), on
every voxel whose n_signal equals the reference's -- on these fixed-seed inputs that is every voxel, and the tests say so.  Eligibility,
the estimate (bit for bit that of k_mppca), the float32 rounding, the pass-through and the scaling by powers of two are exact statements.
No route of k_mppca_denoise has a cap (the eigenvectors live in G's dead triangle, which holds r / 2 of them at every shape), so there is
no input above one: test_no_route_has_a_cap says so for the shapes here, tests/test_mppca_denoise.py for all."""
import functools

import numpy as np
import pytest

import mppca_denoise_np as D
import mppca_np as M
from amico_amd import synthetic as S
from test_mppca import SIGMA
from test_mppca_denoise import C_DEN

pytestmark = pytest.mark.gpu

NAMES = ('sigma', 'signal', 'mean', 'ratio')
SENTINEL = -7.0


def ctx():
    from amico_amd import get_context
    return get_context()


def make_plan(img, mask, b0_idx):
    from amico_amd import _capi
    sel = np.asarray(mask) == 1
    rank = np.full(sel.shape, -1, dtype=np.int32)
    rank[sel] = np.arange(int(sel.sum()), dtype=np.int32)
    return _capi.Prep(ctx(), img.shape, tuple(s // 4 for s in img.strides), rank, [[i] for i in range(img.shape[3])], np.asarray(b0_idx, dtype=np.int32))


def gpu(img, mask, b0_idx, w):
    """-> 'sigma', 'signal', 'mean', 'ratio' [n_vox] of the denoising launch and 'est_*' of amx_prep_noise_mppca_device on the same image,
    'status' [n_vox], 'rows64' [n_vox, nS], 'image' float32 of img's shape and order.  Every output buffer starts as a sentinel and has
    a sentinel tail that must stay"""
    import torch
    plan = make_plan(img, mask, b0_idx)
    nv, nS = plan.n_vox, img.shape[3]
    d = torch.from_numpy(np.array(plan._img_buffer(img))).to('cuda')
    out = torch.full((8, nv), SENTINEL, dtype=torch.float64, device='cuda')
    image = torch.full((plan.extent + 64,), SENTINEL, dtype=torch.float32, device='cuda')
    status = torch.full((nv + 16,), -7, dtype=torch.int32, device='cuda')
    rows = torch.full((nv * nS + 16,), SENTINEL, dtype=torch.float64, device='cuda')
    plan.noise_mppca_denoise_device(d.data_ptr(), w, image.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                    status.data_ptr(), rows.data_ptr())
    assert f'k_mppca_denoise<{w}>' in ctx().last_path().split(' -> ')        # (the path collects the launches of the context)
    plan.noise_mppca_device(d.data_ptr(), w, out[4].data_ptr(), out[5].data_ptr(), out[6].data_ptr(), out[7].data_ptr())
    ctx().sync()
    host = out.cpu().numpy()
    res = {k: host[i] for i, k in enumerate(NAMES)}
    res.update({'est_' + k: host[4 + i] for i, k in enumerate(NAMES)})
    image, status, rows = image.cpu().numpy(), status.cpu().numpy(), rows.cpu().numpy()
    assert (image[plan.extent:] == SENTINEL).all() and (status[nv:] == -7).all() and (rows[nv * nS:] == SENTINEL).all()
    assert np.array_equal(d.cpu().numpy(), plan._img_buffer(img), equal_nan=True)            # the image itself is only read
    res['status'], res['rows64'] = status[:nv], rows[:nv * nS].reshape(nv, nS)
    res['image'] = np.lib.stride_tricks.as_strided(image[:plan.extent], shape=img.shape, strides=img.strides)
    plan.close()
    return res


@functools.lru_cache(maxsize=None)
def case(shape, nS, w, b0=(0,), mask_kind='sphere'):
    """a synthetic image of tests/test_gpu_mppca.py (same seeds), a mask, the reference's answer (made once per case and left alone)"""
    img, mask = M.synthetic(shape, nS, SIGMA, seed=nS + w, b0=b0)
    if mask_kind == 'ones':
        mask = np.ones(shape, dtype=np.uint8)
    elif mask_kind == 'sparse':
        mask = np.random.default_rng(11).choice(np.array([0, 1, 1, 2], dtype=np.uint8), size=shape)     # half of the voxels are columns
    elif mask_kind != 'sphere':
        n_vox = int(mask_kind)
        mask = np.zeros(shape, dtype=np.uint8)
        if n_vox == 1:
            mask[3, 3, 3] = 1
        else:
            mask[1:5, 2:6, 1:5] = 1
            if n_vox == 63:
                mask[1, 2, 1] = 2
            else:
                mask[0, 2, 1] = 1
        assert int((mask == 1).sum()) == n_vox
    img.setflags(write=False)
    return img, mask, D.reference(img, mask, w)


@functools.lru_cache(maxsize=None)
def highrank_case(shape, nS, K, sigma, w):
    img, clean, mask = D.highrank(shape, nS, K, sigma, seed=1)
    img.setflags(write=False)
    return img, mask, D.reference(img, mask, w)


HIGHRANK = {'signal set': ((6, 6, 6), 20, 12, 1.0, 3), 'complement': ((7, 7, 7), 60, 40, 0.3, 5), 'low noise': ((7, 7, 7), 60, 8, 1e-3, 5)}


def check(got, ref, img, mask, max_left_out=0):
    """the per-case assertions of the header; -> the number of voxels left out for a differing n_signal"""
    sel = np.asarray(mask) == 1
    assert np.array_equal(got['status'], ref['status'])
    for k in NAMES:                                               # the estimate is k_mppca's, bit for bit
        assert np.array_equal(got[k].view(np.uint64), got['est_' + k].view(np.uint64)), k
    ok = ref['status'] == 0
    assert np.array_equal(np.isnan(got['sigma']), ~ok)
    assert np.isnan(got['rows64'][~ok]).all() and not np.isnan(got['rows64'][ok]).any()
    # d_out: float32 of the fp64 rows where denoised, the image's bits everywhere else
    expect = np.array(img, dtype=np.float32, order='K', copy=True)
    vox = expect[sel]
    vox[ok] = got['rows64'][ok].astype(np.float32)
    expect[sel] = vox
    assert np.array_equal(got['image'].view(np.uint32), expect.view(np.uint32))
    if not ok.any():
        return 0
    same = ok & (got['signal'] == ref['signal'])
    left_out = int((ok & ~same).sum())
    err = np.linalg.norm(got['rows64'][same] - ref['rows'][same], axis=1)
    b = D.bound(ref, C_DEN)[same]
    zero = ref['signal'][same] == 0
    nz = ~zero
    with np.errstate(invalid='ignore', divide='ignore'):
        worst = float(np.max(err[nz] / b[nz])) if nz.any() else 0.0
    print(f'{img.shape}: {int(ok.sum())} of {len(ok)} voxels denoised, n_signal {int(np.nanmin(ref["signal"]))}..{int(np.nanmax(ref["signal"]))}, '
          f'left out {left_out}; row error / bound: max {worst:.3e}; relative row error: max {np.max(err / ref["norm"][same]):.2e}; '
          f'margin min {np.nanmin(ref["margin"]):.2e}')
    assert left_out <= max_left_out and left_out <= 0.01 * ok.sum()
    assert np.all(err[nz] <= b[nz])
    assert (got['rows64'][same][zero] == 0.0).all()              # s = 0: the rank-0 reconstruction
    return left_out


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize('nS', [20, 27, 32, 15, 16, 17])
def test_w3(nS):
    """m < n, m = n, m > n at a full patch; r = 15, 16, 17 across the MFMA tile edge"""
    img, mask, ref = case((10, 10, 10), nS, 3, b0=(0, 3))
    check(gpu(img, mask, (0, 3), 3), ref, img, mask)


@pytest.mark.parametrize('shape,nS', [((9, 9, 9), 40), ((8, 8, 8), 130), ((7, 7, 7), 512)])
def test_w5(shape, nS):
    img, mask, ref = case(shape, nS, 5)
    check(gpu(img, mask, (0,), 5), ref, img, mask)


@pytest.mark.parametrize('shape,nS,w', [((3, 6, 5), 20, 3), ((5, 5, 5), 70, 5)])
def test_axis_of_exactly_the_patch(shape, nS, w):
    img, mask, ref = case(shape, nS, w, mask_kind='ones')
    assert (ref['status'] == 0).all()
    check(gpu(img, mask, (0,), w), ref, img, mask)


@pytest.mark.parametrize('shape,nS,w', [((10, 10, 10), 20, 3), ((9, 9, 9), 40, 5), ((8, 8, 8), 130, 5)])
def test_fortran_order_image(shape, nS, w):
    """the volume axis slowest: the columns come in another order, the centre's column is another index"""
    img, mask, ref = case(shape, nS, w)
    imgf = np.asfortranarray(img)
    assert imgf.strides[0] == 4 and imgf.strides[3] > imgf.strides[2]
    got = gpu(imgf, mask, (0,), w)
    assert got['image'].strides == imgf.strides
    check(got, ref, imgf, mask)


def test_sparse_mask_on_both_sides_of_the_threshold():
    img, mask, ref = case((8, 9, 7), 20, 3, mask_kind='sparse')
    assert 0.2 < (ref['status'] == 1).mean() < 0.8 and (mask == 2).any()
    check(gpu(img, mask, (0,), 3), ref, img, mask)


@pytest.mark.parametrize('n_vox', [1, 63, 65])
def test_few_voxels(n_vox):
    """one workgroup of patches and a bit; a single voxel has no patch and is passed through"""
    img, mask, ref = case((6, 7, 6), 20, 3, mask_kind=str(n_vox))
    assert (ref['status'] == 1).all() == (n_vox == 1)
    check(gpu(img, mask, (0,), 3), ref, img, mask)


@pytest.mark.parametrize('name', list(HIGHRANK))
def test_high_rank(name):
    """K profiles mixed at random per voxel: the signal set is taken (s of about 3 to 8 of 20), the complement (s of 37 to 40 of 60: the
    20 or so noise vectors are made and the projection subtracted), and sigma = 1e-3 on amplitude 100 (lambda_max / gap of 3e11)"""
    shape, nS, K, sigma, w = HIGHRANK[name]
    img, mask, ref = highrank_case(*HIGHRANK[name])
    s, r = ref['signal'], ref['r']
    if name == 'complement':
        assert (2 * s > r).all() and s.min() >= 30
    else:
        assert (2 * s <= r).all() and s.max() >= 8
    check(gpu(img, mask, (0,), w), ref, img, mask)


def test_no_route_has_a_cap():
    from amico_amd import _capi
    for (shape, nS, w) in [((10, 10, 10), 20, 3), ((9, 9, 9), 40, 5), ((8, 8, 8), 130, 5), ((7, 7, 7), 512, 5), ((7, 7, 7), 60, 5)]:
        rt = _capi.mppca_denoise_route(nS, w, w ** 3, shape)
        assert rt['cap'] == 0 and rt['capacity'] >= rt['r'] // 2 and rt['lds'] <= 160 * 1024


# ------------------------------------------------------------------ the whole file
@pytest.mark.parametrize('w,nS', [(3, 20), (5, 40)])
def test_one_nan_and_one_inf_sample(w, nS):
    """exactly the centres whose cube holds the sample are passed through, their own non-finite sample copied as it is; every other voxel
    meets the reference"""
    shape = (9, 9, 9)
    base, _, _ = case(shape, nS, w)
    img = base.copy()
    mask = np.ones(shape, dtype=np.uint8)
    bad = [((1, 4, 7), 5, np.nan), ((6, 2, 3), nS - 1, np.inf)]
    for vox, vol, value in bad:
        img[vox + (vol,)] = value
    hit = np.zeros(shape, dtype=bool)
    for c in np.argwhere(mask == 1):
        s = [M.cube_start(int(c[a]), shape[a], w) for a in range(3)]
        hit[tuple(c)] = any(all(s[a] <= vox[a] < s[a] + w for a in range(3)) for vox, _, _ in bad)
    got = gpu(img, mask, (0,), w)
    assert 0 < hit.sum() < hit.size and np.array_equal(got['status'], hit.ravel().astype(np.int32))
    assert np.isnan(got['image'][1, 4, 7, 5]) and np.isposinf(got['image'][6, 2, 3, nS - 1])
    assert np.array_equal(got['image'][hit].view(np.uint32), img[hit].view(np.uint32))
    check(got, D.reference(img, mask, w), img, mask)


@pytest.mark.parametrize('shape,nS,w', [((10, 10, 10), 27, 3), ((10, 10, 10), 32, 3), ((9, 9, 9), 40, 5), ((8, 8, 8), 130, 5)])
def test_scale_by_powers_of_two_is_exact(shape, nS, w):
    img, mask, _ = case(shape, nS, w, b0=(0, 3))
    one = gpu(img, mask, (0, 3), w)
    for k in (-10, 14):
        f = np.float32(2.0 ** k)
        scaled = img * f
        assert np.array_equal(scaled / f, img)
        got = gpu(scaled, mask, (0, 3), w)
        assert np.array_equal(got['status'], one['status'])
        assert np.array_equal(got['rows64'], one['rows64'] * 2.0 ** k, equal_nan=True)
        assert np.array_equal(got['image'], one['image'] * f)
        assert np.array_equal(got['signal'], one['signal'], equal_nan=True) and np.array_equal(got['sigma'], one['sigma'] * 2.0 ** k, equal_nan=True)


def test_arguments_come_back_through_amx_bad():
    import torch
    from amico_amd import _capi
    c = ctx()
    shape, nS = (6, 6, 6), 12
    img, _, _ = case(shape, nS, 3)
    rank = np.arange(216, dtype=np.int32).reshape(shape)
    groups = [[i] for i in range(nS)]
    st = tuple(s // 4 for s in img.strides)
    plan = _capi.Prep(c, img.shape, st, rank, groups, [0])
    d = torch.from_numpy(np.array(img)).to('cuda')
    out = torch.full((plan.extent + 8,), SENTINEL, dtype=torch.float32, device='cuda')
    o = torch.full((216 * 8,), SENTINEL, dtype=torch.float64, device='cuda')
    p0, po = o.data_ptr(), out.data_ptr()
    with pytest.raises(ValueError, match='not a plan'):
        c.check(_capi.lib().amx_prep_noise_mppca_denoise_device(c._h, None, d.data_ptr(), 3, po, None, None, None, None, None, None, None))
    for patch in (4, 7, 0, -3):
        with pytest.raises(ValueError, match='patch edge must be 3 or 5'):
            plan.noise_mppca_denoise_device(d.data_ptr(), patch, po)
    with pytest.raises(ValueError, match='null buffer'):
        plan.noise_mppca_denoise_device(d.data_ptr(), 3, 0, p0)
    with pytest.raises(ValueError, match='null buffer'):
        plan.noise_mppca_denoise_device(0, 3, po)
    for bad_out in (d.data_ptr(), d.data_ptr() + 4 * (plan.extent - 1), d.data_ptr() - 4 * (plan.extent - 1)):
        with pytest.raises(ValueError, match='overlaps the image'):
            plan.noise_mppca_denoise_device(d.data_ptr(), 3, bad_out)
    for other in (dict(d_sigma=po), dict(d_sigma=p0, d_mean=p0), dict(d_sigma=p0, d_status=p0 + 8 * 215), dict(d_ratio=p0 + 8, d_rows64=p0 + 216 * 8 - 8 * 216 * nS),
                  dict(d_status=d.data_ptr() + 4)):
        with pytest.raises(ValueError, match='overlap'):
            plan.noise_mppca_denoise_device(d.data_ptr(), 3, po, **other)
    plan.noise_mppca_denoise_device(d.data_ptr(), 3, po, p0, d_ratio=p0 + 8 * 216)            # adjacent is not overlapping
    short = _capi.Prep(c, (6, 4, 6, nS), (4 * 6 * nS, 6 * nS, nS, 1), np.arange(144, dtype=np.int32).reshape(6, 4, 6), groups, [0])
    with pytest.raises(ValueError, match='shorter than the patch'):
        short.noise_mppca_denoise_device(d.data_ptr(), 5, po)
    empty = _capi.Prep(c, img.shape, st, np.full(shape, -1, dtype=np.int32), groups, [0])
    with pytest.raises(ValueError, match='no masked voxel'):
        empty.noise_mppca_denoise_device(d.data_ptr(), 3, po)
    c.sync()
    host, image = o.cpu().numpy(), out.cpu().numpy()
    assert not (host[:216 * 2] == SENTINEL).any() and (host[216 * 2:] == SENTINEL).all()
    assert not (image[:plan.extent] == SENTINEL).any() and (image[plan.extent:] == SENTINEL).all()
    for p in (plan, short, empty):
        p.close()


def test_denoise_mppca_numpy_in_numpy_out():
    from amico_amd import noise
    shape, nS, w = (9, 9, 9), 40, 5
    img, mask, ref = case(shape, nS, w)
    got = gpu(img, mask, (0,), w)
    for arr in (img, np.asfortranarray(img)):
        res = noise.denoise_mppca(arr, mask, [0], patch=w)
        assert set(res) == {'snr', 'sigma', 'voxels', 'mean', 'sd', 'signal', 'image', 'status', 'denoised', 'passed_through'}
        assert res['image'].dtype == np.float32 and res['image'].shape == arr.shape and res['image'].strides == arr.strides
        assert np.array_equal(res['image'], got['image']) and np.array_equal(res['status'], ref['status'])
        assert res['denoised'] == int((ref['status'] == 0).sum()) == res['voxels']
        assert res['denoised'] + res['passed_through'] == int((mask == 1).sum())
        # the estimate is that of the estimator on the same array (another order of the columns rounds the sums another way)
        est = noise.estimate_mppca(arr, mask, [0], patch=w)
        for k in ('snr', 'sigma', 'voxels'):
            assert res[k] == est[k]
        for k in ('mean', 'sd', 'signal'):
            assert np.array_equal(res[k], est[k], equal_nan=True)
    with pytest.raises(ValueError, match='noise_patch'):
        noise.denoise_mppca(img, mask, [0], patch=4)
    with pytest.raises(RuntimeError, match='noise_patch'):
        noise.denoise_mppca(img[:, :4], mask[:, :4], [0], patch=5)


# ------------------------------------------------------------------ Evaluation
@pytest.fixture(scope='module')
def brain(htable500):
    """the fixture of tests/test_gpu_mppca.py: 16 x 16 x 8 voxels, ONE b0 volume and one shell of 30 directions at b = 1000, NODDI signals
    at SNR 20 on smoothly varying amplitudes around 1000, Fortran order, a mask of 0 / 1 / 2 that is mostly 1"""
    shape = (16, 16, 8)
    n = int(np.prod(shape))
    sch = S.make_scheme(1, ((1000.0, 30),), seed=2)
    assert sch.b0_count == 1
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
    return {'sch': sch, 'K': K, 'ht': ht, 'img': np.asfortranarray(img), 'mask': mask, 'sigma': sg}


def run(brain, img=None, mask=None, **config):
    import amico_amd
    ae = amico_amd.Evaluation()
    for key, value in config.items():
        ae.set_config(key.replace('DWI_SNR', 'DWI-SNR'), value)
    ae.set_data(brain['img'] if img is None else img, brain['sch'], brain['mask'] if mask is None else mask)
    ae.set_model('NODDI')
    ae.set_kernels(brain['K'], brain['ht'])
    ae.fit()
    return ae


KEYS = ('MAPs', 'DIRs', 'DTI_outliers', 'DTI_MAPs', 'DTI_evals')


def test_evaluation_denoise_is_the_fit_of_the_denoised_image(brain):
    """(A) doDenoise, debias and RESTORE with no number given; (B) no denoise key, the image of noise.denoise_mppca, DWI-SNR = what (A)
    reported: the same bits everywhere.  DWI_denoised is that image, NOISE_MAPs those of doEstimateNoise = 'MPPCA'"""
    from amico_amd import noise
    a = run(brain, doDenoise='mppca', doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True, doSaveDenoisedDWI=True)
    snr = a.get_config('DWI-SNR_estimated')
    assert a.get_config('noise_method') == 'MPPCA' and a.get_config('DWI-SNR') is None and a.get_config('DTI_sigma') is None
    den = noise.denoise_mppca(brain['img'], brain['mask'], brain['sch'].b0_idx, patch=5)
    assert snr == den['snr'] and a.get_config('noise_sigma_estimated') == den['sigma'] and a.get_config('noise_voxels') == den['voxels']
    assert a.get_config('denoise_voxels') == den['denoised'] > 0
    assert a.get_config('denoise_passed_through') == den['passed_through'] == int((brain['mask'] == 1).sum()) - den['denoised']
    got = a.RESULTS['DWI_denoised']
    assert got.dtype == np.float32 and got.shape == brain['img'].shape and np.array_equal(got.view(np.uint32), den['image'].view(np.uint32))
    sel = brain['mask'] == 1
    assert not np.array_equal(got[sel], brain['img'][sel]) and np.array_equal(got[~sel], brain['img'][~sel])
    b = run(brain, img=den['image'], doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True, DWI_SNR=snr)
    for key in KEYS:
        assert np.array_equal(a.RESULTS[key].view(np.uint32), b.RESULTS[key].view(np.uint32)), key
    assert tuple(a.get_config('dti_robust')) == tuple(b.get_config('dti_robust')) and np.array_equal(a.y, b.y)
    assert 'DWI_denoised' not in b.RESULTS and b.get_config('denoise_voxels') is None
    # the estimate is the one doEstimateNoise = 'MPPCA' makes of the raw image, and asking for both launches nothing twice
    e = run(brain, doEstimateNoise='MPPCA')
    both = run(brain, doDenoise=True, doEstimateNoise='MPPCA', doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True)
    assert np.array_equal(a.RESULTS['NOISE_MAPs'], e.RESULTS['NOISE_MAPs']) and e.get_config('DWI-SNR_estimated') == snr
    for key in KEYS + ('NOISE_MAPs',):
        assert np.array_equal(a.RESULTS[key].view(np.uint32), both.RESULTS[key].view(np.uint32)), key
    assert 'DWI_denoised' not in both.RESULTS


def test_evaluation_without_the_key_nothing_moves(brain):
    plain = run(brain)
    assert 'DWI_denoised' not in plain.RESULTS and 'NOISE_MAPs' not in plain.RESULTS
    assert plain.get_config('doDenoise') is False and plain.get_config('doSaveDenoisedDWI') is False
    for key in ('denoise_voxels', 'denoise_passed_through', 'noise_method', 'DWI-SNR_estimated'):
        assert key not in plain.CONFIG
    d = run(brain, doDenoise=True, doSaveDenoisedDWI=True)
    assert set(d.RESULTS) - set(plain.RESULTS) == {'NOISE_MAPs', 'DWI_denoised'} and not np.array_equal(d.RESULTS['MAPs'], plain.RESULTS['MAPs'])
    d.set_config('doDenoise', False)                             # the same Evaluation once more without the key: nothing lingers
    d.set_data(brain['img'], brain['sch'], brain['mask'])
    d.fit()
    assert set(d.RESULTS) == set(plain.RESULTS) and np.array_equal(d.RESULTS['MAPs'].view(np.uint32), plain.RESULTS['MAPs'].view(np.uint32))
    assert 'noise_method' not in d.CONFIG and 'denoise_voxels' not in d.CONFIG and 'denoise_passed_through' not in d.CONFIG
    for value in ('PCA', 1, 'yes'):
        with pytest.raises(ValueError, match='doDenoise'):
            run(brain, doDenoise=value)
    with pytest.raises(RuntimeError, match='noise_patch'):
        run(brain, img=brain['img'][:, :, :4], mask=brain['mask'][:, :, :4], doDenoise=True)


def test_evaluation_patch_3_and_without_normalisation(brain):
    from amico_amd import noise
    a = run(brain, doDenoise='MPPCA', noise_patch=3, doSaveDenoisedDWI=True)
    den = noise.denoise_mppca(brain['img'], brain['mask'], brain['sch'].b0_idx, patch=3)
    assert a.get_config('noise_patch') == 3 and np.array_equal(a.RESULTS['DWI_denoised'], den['image'])
    b = run(brain, img=den['image'])
    assert np.array_equal(a.RESULTS['MAPs'].view(np.uint32), b.RESULTS['MAPs'].view(np.uint32)) and np.array_equal(a.y, b.y)
    a = run(brain, doDenoise='MPPCA', doNormalizeSignal=False, DTI_fit_method='RESTORE', doSaveTensorMaps=True)
    den = noise.denoise_mppca(brain['img'], brain['mask'], brain['sch'].b0_idx, patch=5)
    b = run(brain, img=den['image'], doNormalizeSignal=False, DTI_fit_method='RESTORE', doSaveTensorMaps=True, DTI_sigma=a.get_config('noise_sigma_estimated'))
    for key in KEYS:
        assert np.array_equal(a.RESULTS[key].view(np.uint32), b.RESULTS[key].view(np.uint32)), key
    assert np.array_equal(a.y, b.y)


def test_evaluation_no_eligible_voxel_is_the_existing_error(brain):
    mask = np.zeros_like(brain['mask'])
    mask[::3, ::3, ::3] = 1                                       # no cube holds half of its voxels
    with pytest.raises(RuntimeError, match='doEstimateNoise: no voxel of the mask has a patch'):
        run(brain, mask=mask, doDenoise=True)
