"""The Marchenko-Pastur noise estimator on the GPU (k_mppca, amx_prep_noise_mppca_device; doEstimateNoise = 'MPPCA') against its
numpy restatement (tests/mppca_np.py: cube, columns, eligibility, Gram matrix, numpy.linalg.eigvalsh, the rule).

Bounds.  An eigenvalue may differ from the reference's by  d = C_EIG eps (q + r) lambda_max  of its own voxel (C_EIG = 0.72: four times the
worst constant the restated algorithm showed against a long-double Gram matrix, tests/test_mppca.py).  sigma^2 = S_p / ((p+1) q) is a mean of
p+1 eigenvalues over q, so its relative error is at most B = d / (q sigma^2), sigma's B / 2 plus the roundings of the rule itself (four ulp).
sigma and n_signal are held on every voxel whose decision margin (the smallest |s2 - s1| / s1 over p) exceeds 2 B; on the fixed-seed
inputs here that is every voxel, and the tests say so.  Eligibility, the b0 mean and the scaling by powers of two are exact statements."""
import functools

import numpy as np
import pytest

import mppca_np as M
from amico_amd import synthetic as S
from test_mppca import C_EIG, EPS, SIGMA

pytestmark = pytest.mark.gpu

NAMES = ('sigma', 'signal', 'mean', 'ratio')


def ctx():
    from amico_amd import get_context
    return get_context()


def gpu(img, mask, b0_idx, w):
    """-> dict of numpy arrays: 'sigma', 'signal', 'mean', 'ratio' [n_vox], 'eig' [n_vox, 125], and the plan's b0 estimator's 'b0_mean'
    when the scheme has two b0 volumes or more"""
    import torch
    from amico_amd import _capi
    sel = np.asarray(mask) == 1
    rank = np.full(sel.shape, -1, dtype=np.int32)
    rank[sel] = np.arange(int(sel.sum()), dtype=np.int32)
    plan = _capi.Prep(ctx(), img.shape, tuple(s // 4 for s in img.strides), rank, [[i] for i in range(img.shape[3])], np.asarray(b0_idx, dtype=np.int32))
    nv = plan.n_vox
    d = torch.from_numpy(np.array(plan._img_buffer(img))).to('cuda')
    out = torch.full((5, nv), -7.0, dtype=torch.float64, device='cuda')
    eig = torch.full((nv, M.MAX_SIDE), -7.0, dtype=torch.float64, device='cuda')
    plan.noise_mppca_device(d.data_ptr(), w, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), eig.data_ptr())
    if len(b0_idx) >= 2:
        plan.noise_b0_device(d.data_ptr(), out[4].data_ptr())
    ctx().sync()
    host = out.cpu().numpy()
    res = {k: host[i] for i, k in enumerate(NAMES)}
    res['b0_mean'] = host[4]
    res['eig'] = eig.cpu().numpy()
    plan.close()
    return res


@functools.lru_cache(maxsize=None)
def case(shape, nS, w, seed=None, b0=(0,), order='C'):
    """a synthetic image, its mask, the reference's answer (made once per case and left alone)"""
    img, mask = M.synthetic(shape, nS, SIGMA, seed=nS + w if seed is None else seed, b0=b0)
    img = np.asarray(img, order=order)
    img.setflags(write=False)
    return img, mask, M.estimate(img, mask, b0, w)


def check(got, ref, nS, w, shape, b0=(0,), max_left_out=0):
    """eligibility exact; eigenvalues, sigma and n_signal within the bounds of the header; the mean bit for bit; the route of every patch"""
    from amico_amd import _capi
    nan_ref = np.isnan(ref['sigma'])
    for k in ('sigma', 'signal', 'ratio') + (('mean',) if len(b0) else ()):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
    assert np.array_equal(np.isnan(got['eig']), np.isnan(ref['eig']))
    ok = ~nan_ref
    assert np.array_equal(got['mean'], ref['mean'], equal_nan=True)
    if len(b0) >= 2:
        both = ok & ~np.isnan(got['b0_mean'])
        assert both.any() and np.array_equal(got['mean'][both].view(np.uint64), got['b0_mean'][both].view(np.uint64))
    if not ok.any():
        return 0
    for n in np.unique(ref['n']).astype(int):          # what the launch arithmetic says of every patch size met
        rt = _capi.mppca_route(nS, w, n, shape)
        at = ref['n'] == n
        assert rt['r'] == ref['r'][at][0] and rt['q'] == ref['q'][at][0] and rt['side'] == ('volumes' if nS <= n else 'patch')
        assert rt['eligible'] == (2 * n >= w ** 3) and rt['lds'] <= 160 * 1024
        assert not (ok & at).any() or rt['eligible']
    q, r = ref['q'][ok], ref['r'][ok]
    d = C_EIG * EPS * (q + r) * ref['lam_max'][ok]
    err = np.nanmax(np.abs(got['eig'][ok] - ref['eig'][ok]), axis=1)
    print(f'{shape} x {nS}, w {w}: {int(ok.sum())} of {len(ok)} voxels eligible, r {int(r.min())}..{int(r.max())}, q {int(q.min())}..{int(q.max())}; '
          f'eigenvalue error / bound: max {np.max(err / d):.3f}')
    assert np.all(err <= d)
    B = d / (q * ref['sigma'][ok] ** 2)
    held = ref['margin'][ok] > 2 * B
    left_out = int((~held).sum())
    rel = np.abs(got['sigma'][ok] / ref['sigma'][ok] - 1.0)
    print(f'    margin: min {ref["margin"][ok].min():.2e} against 2 B of at most {2 * B.max():.2e}; left out {left_out}; '
          f'sigma error / bound: max {np.max(rel[held] / (B[held] / 2 + 4 * EPS)):.3f}')
    assert left_out <= max_left_out and left_out <= 0.01 * ok.sum()
    assert np.all(rel[held] <= B[held] / 2 + 4 * EPS)
    assert np.array_equal(got['signal'][ok][held], ref['signal'][ok][held])
    ratio = got['mean'][ok] / got['sigma'][ok]
    assert np.array_equal(got['ratio'][ok], ratio, equal_nan=True)
    return left_out


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize('nS,side', [(20, 'volumes'), (27, 'volumes'), (32, 'patch'), (15, 'volumes'), (16, 'volumes'), (17, 'volumes')])
def test_w3(nS, side):
    """m < n, m = n, m > n at a full patch; r = 15, 16, 17 across the MFMA tile edge; q = 27 is no multiple of 4"""
    from amico_amd import _capi
    shape = (10, 10, 10)
    img, mask, ref = case(shape, nS, 3, b0=(0, 3))
    rt = _capi.mppca_route(nS, 3, 27, shape)
    assert rt['side'] == side and rt['waves'] == 1 and rt['patches'] == 4 and rt['r'] == min(nS, 27) and rt['q'] == max(nS, 27)
    assert 27.0 in ref['n'] and (nS >= 27 or rt['q'] % 4 != 0)
    check(gpu(img, mask, (0, 3), 3), ref, nS, 3, shape, b0=(0, 3))


@pytest.mark.parametrize('shape,nS,r_full,side', [((9, 9, 9), 40, 40, 'volumes'), ((8, 8, 8), 130, 125, 'patch'), ((7, 7, 7), 512, 125, 'patch')])
def test_w5(shape, nS, r_full, side):
    from amico_amd import _capi
    img, mask, ref = case(shape, nS, 5)
    rt = _capi.mppca_route(nS, 5, 125, shape)
    assert rt['side'] == side and rt['r'] == r_full and rt['waves'] == 4 and rt['patches'] == 1
    assert 125.0 in ref['n'] and len(np.unique(ref['n'])) > 1          # full patches and patches the spherical mask cuts
    check(gpu(img, mask, (0,), 5), ref, nS, 5, shape)


@pytest.mark.parametrize('shape,nS,w', [((3, 6, 5), 20, 3), ((7, 5, 6), 12, 5), ((5, 5, 5), 70, 5)])
def test_axis_of_exactly_the_patch(shape, nS, w):
    """every cube along that axis is the whole axis; q = 27 / 125 / 125, the last with r = 70 (no multiple of 16, q no multiple of 4)"""
    img, _, _ = case(shape, nS, w)
    mask = np.ones(shape, dtype=np.uint8)
    ref = M.estimate(img, mask, (0,), w)
    assert not np.isnan(ref['sigma']).any()
    check(gpu(img, mask, (0,), w), ref, nS, w, shape)


@pytest.mark.parametrize('shape,nS,w', [((10, 10, 10), 20, 3), ((9, 9, 9), 40, 5), ((8, 8, 8), 130, 5)])
def test_fortran_order_image(shape, nS, w):
    """the volume axis slowest (nibabel's layout): the memory axes are the spatial axes reversed, the columns come in another order"""
    img, mask, ref = case(shape, nS, w)
    imgf = np.asfortranarray(img)
    assert imgf.strides[0] == 4 and imgf.strides[3] > imgf.strides[2]
    got = gpu(imgf, mask, (0,), w)
    check(got, ref, nS, w, shape)


def test_sparse_mask_on_both_sides_of_the_threshold():
    shape, nS, w = (8, 9, 7), 20, 3
    img, _, _ = case(shape, nS, w)
    mask = np.random.default_rng(11).choice(np.array([0, 1, 1, 2], dtype=np.uint8), size=shape)     # half of the voxels are columns
    ref = M.estimate(img, mask, (0,), w)
    n = ref['n']
    assert (n == 13).any() and (n == 14).any() and 0.2 < np.isnan(ref['sigma']).mean() < 0.8    # 2 n >= 27 <=> n >= 14
    assert np.array_equal(np.isnan(ref['sigma']), n < 14)
    check(gpu(img, mask, (0,), w), ref, nS, w, shape)


@pytest.mark.parametrize('w,nS', [(3, 20), (5, 40)])
def test_one_nan_and_one_inf_sample(w, nS):
    """exactly the centres whose cube holds the sample are NaN, and no other"""
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
    assert 0 < hit.sum() < hit.size
    for k in ('sigma', 'signal', 'mean', 'ratio'):
        assert np.array_equal(np.isnan(got[k]), hit.ravel()), k
    assert np.array_equal(np.isnan(got['eig']).all(axis=1), hit.ravel())
    check(got, M.estimate(img, mask, (0,), w), nS, w, shape)


@pytest.mark.parametrize('n_vox', [1, 63, 65])
def test_few_voxels(n_vox):
    """one workgroup of patches and a bit: a 4 x 4 x 4 block of the mask less one voxel, or plus one; a single voxel has no patch"""
    shape, nS, w = (6, 7, 6), 20, 3
    img, _, _ = case(shape, nS, w)
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
    ref = M.estimate(img, mask, (0,), w)
    assert np.isnan(ref['sigma']).all() == (n_vox == 1)
    check(gpu(img, mask, (0,), w), ref, nS, w, shape)


@pytest.mark.parametrize('shape,nS,w', [((10, 10, 10), 27, 3), ((10, 10, 10), 32, 3), ((9, 9, 9), 40, 5), ((8, 8, 8), 130, 5)])
def test_scale_by_powers_of_two_is_exact(shape, nS, w):
    """amplitudes 2^-10 and 2^14: the outputs are 2^k times those of the image itself, bit for bit; n_signal, the ratio and the NaN
    pattern do not move; and the scaled images meet the reference like any other"""
    img, mask, ref = case(shape, nS, w, b0=(0, 3))
    one = gpu(img, mask, (0, 3), w)
    for k in (-10, 14):
        f = np.float32(2.0 ** k)
        scaled = img * f
        assert np.array_equal(scaled / f, img)
        got = gpu(scaled, mask, (0, 3), w)
        assert np.array_equal(got['sigma'], one['sigma'] * 2.0 ** k, equal_nan=True)
        assert np.array_equal(got['mean'], one['mean'] * 2.0 ** k, equal_nan=True)
        assert np.array_equal(got['eig'], one['eig'] * 4.0 ** k, equal_nan=True)
        assert np.array_equal(got['signal'], one['signal'], equal_nan=True) and np.array_equal(got['ratio'], one['ratio'], equal_nan=True)
        if k == 14 and w == 3:
            check(got, M.estimate(scaled, mask, (0, 3), w), nS, w, shape, b0=(0, 3))


# ------------------------------------------------------------------ arguments
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
    o = torch.full((216 * 128,), -7.0, dtype=torch.float64, device='cuda')      # sigma [216], ratio [216], eig [216 x 125], 216 spare
    p0 = o.data_ptr()
    with pytest.raises(ValueError, match='not a plan'):
        c.check(_capi.lib().amx_prep_noise_mppca_device(c._h, None, d.data_ptr(), 3, p0, None, None, None, None, None))
    for patch in (4, 7, 0, -3):
        with pytest.raises(ValueError, match='patch edge must be 3 or 5'):
            plan.noise_mppca_device(d.data_ptr(), patch, p0)
    with pytest.raises(ValueError, match='at least one'):
        plan.noise_mppca_device(d.data_ptr(), 3)
    with pytest.raises(ValueError, match='null buffer'):
        plan.noise_mppca_device(0, 3, p0)
    for other in (dict(d_mean=p0), dict(d_ratio=p0 + 8 * 215), dict(d_eig=p0 - 8 * 125 * 216 + 8), dict(d_nsignal=p0 + 8, d_eig=p0 + 216 * 8)):
        with pytest.raises(ValueError, match='overlap'):
            plan.noise_mppca_device(d.data_ptr(), 3, p0, **other)
    plan.noise_mppca_device(d.data_ptr(), 3, p0, d_ratio=p0 + 8 * 216, d_eig=p0 + 8 * 432)      # adjacent is not overlapping
    short = _capi.Prep(c, (6, 4, 6, nS), (4 * 6 * nS, 6 * nS, nS, 1), np.arange(144, dtype=np.int32).reshape(6, 4, 6), groups, [0])
    with pytest.raises(ValueError, match='shorter than the patch'):
        short.noise_mppca_device(d.data_ptr(), 5, p0)
    empty = _capi.Prep(c, img.shape, st, np.full(shape, -1, dtype=np.int32), groups, [0])
    with pytest.raises(ValueError, match='no masked voxel'):
        empty.noise_mppca_device(d.data_ptr(), 3, p0)
    c.sync()
    host = o.cpu().numpy()
    assert not (host[:216 * 127] == -7.0).any() and (host[216 * 127:] == -7.0).all()
    for p in (plan, short, empty):
        p.close()


def test_estimate_mppca_numpy_in_numpy_out():
    from amico_amd import noise
    shape, nS, w = (9, 9, 9), 40, 5
    img, mask, ref = case(shape, nS, w)
    res = noise.estimate_mppca(img, mask, [0], patch=w)
    assert set(res) == {'snr', 'sigma', 'voxels', 'mean', 'sd', 'signal'}
    got = gpu(img, mask, (0,), w)
    assert np.array_equal(res['sd'], got['sigma'], equal_nan=True) and np.array_equal(res['signal'], got['signal'], equal_nan=True)
    assert np.array_equal(res['mean'], got['mean'], equal_nan=True)
    assert res['voxels'] == int((~np.isnan(ref['sigma'])).sum())
    assert res['sigma'] == np.nanmedian(got['sigma']) and res['snr'] == np.nanmedian(got['ratio'])
    assert 0.94 <= res['sigma'] / SIGMA <= 1.02                     # the band of tests/test_mppca.py
    nob0 = noise.estimate_mppca(img, mask, [], patch=w)
    assert np.isnan(nob0['snr']) and nob0['sigma'] == res['sigma'] and np.isnan(nob0['mean']).all()
    with pytest.raises(ValueError, match='noise_patch'):
        noise.estimate_mppca(img, mask, [0], patch=4)
    with pytest.raises(RuntimeError, match='noise_patch'):
        noise.estimate_mppca(img[:, :4], mask[:, :4], [0], patch=5)


# ------------------------------------------------------------------ Evaluation
@pytest.fixture(scope='module')
def brain(htable500):
    """16 x 16 x 8 voxels, ONE b0 volume and one shell of 30 directions at b = 1000, NODDI signals at SNR 20 on smoothly varying
    amplitudes around 1000, Fortran order, a mask of 0 / 1 / 2 that is mostly 1"""
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


def run(brain, **config):
    import amico_amd
    ae = amico_amd.Evaluation()
    for key, value in config.items():
        ae.set_config(key.replace('DWI_SNR', 'DWI-SNR'), value)
    ae.set_data(brain['img'], brain['sch'], brain['mask'])
    ae.set_model('NODDI')
    ae.set_kernels(brain['K'], brain['ht'])
    ae.fit()
    return ae


RESTORE_KEYS = ('MAPs', 'DIRs', 'DTI_outliers', 'DTI_MAPs', 'DTI_evals')


def test_evaluation_single_b0_end_to_end(brain):
    """(A) 'MPPCA', debias and RESTORE with no number given on a scheme with one b0 -- the b0 estimator refuses it; (B) no key, DWI-SNR =
    what (A) reported: the same bits everywhere.  NOISE_MAPs = b0 mean, sigma, signal components: the scatter of the rows"""
    from amico_amd import noise
    with pytest.raises(RuntimeError, match='b0 repeats'):
        run(brain, doEstimateNoise=True)
    a = run(brain, doEstimateNoise='mppca', doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True)
    snr, sigma, c = a.get_config('DWI-SNR_estimated'), a.get_config('noise_sigma_estimated'), a.get_config('noise_voxels')
    print(f'estimated SNR {snr:.3f}, sigma {sigma:.3f} (made with 50 on amplitudes around 1000), {c} voxels')
    assert a.get_config('noise_method') == 'MPPCA' and a.get_config('noise_patch') == 5
    assert a.get_config('DWI-SNR') is None and a.get_config('DTI_sigma') is None
    # a sanity bound, not the accuracy test: the band of tests/test_mppca.py widened by the Rician floor of the attenuated samples
    assert 0 < c <= int((brain['mask'] == 1).sum()) and 0.85 * brain['sigma'] < sigma < 1.05 * brain['sigma'] and 10.0 < snr < 40.0
    b = run(brain, doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True, DWI_SNR=snr)
    assert 'NOISE_MAPs' not in b.RESULTS and b.get_config('DWI-SNR_estimated') is None and b.get_config('noise_method') is None
    for key in RESTORE_KEYS:
        assert np.array_equal(a.RESULTS[key].view(np.uint32), b.RESULTS[key].view(np.uint32)), key
    assert tuple(a.get_config('dti_robust')) == tuple(b.get_config('dti_robust')) and np.array_equal(a.y, b.y)
    rows = noise.estimate_mppca(brain['img'], brain['mask'], brain['sch'].b0_idx, patch=5)
    assert rows['snr'] == snr and rows['sigma'] == sigma and rows['voxels'] == c
    sel = brain['mask'] == 1
    vol = np.zeros(sel.shape + (3,), dtype=np.float32)
    for ch, k in enumerate(('mean', 'sd', 'signal')):
        vol[sel, ch] = np.nan_to_num(rows[k], nan=0.0).astype(np.float32)
    got = a.RESULTS['NOISE_MAPs']
    assert got.dtype == np.float32 and got.shape == vol.shape and np.array_equal(got, vol) and (vol[..., 1] > 0).sum() == c


def test_evaluation_patch_3_and_without_normalisation(brain):
    """noise_patch 3; doNormalizeSignal off: `y` is in image units and (B) is handed DTI_sigma = noise_sigma_estimated"""
    a = run(brain, doEstimateNoise='MPPCA', noise_patch=3, doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True,
            doNormalizeSignal=False)
    snr, sigma = a.get_config('DWI-SNR_estimated'), a.get_config('noise_sigma_estimated')
    assert 0.80 * brain['sigma'] < sigma < 1.05 * brain['sigma']
    b = run(brain, doDebiasSignal=True, DTI_fit_method='RESTORE', doSaveTensorMaps=True, doNormalizeSignal=False, DWI_SNR=snr, DTI_sigma=sigma)
    for key in RESTORE_KEYS:
        assert np.array_equal(a.RESULTS[key].view(np.uint32), b.RESULTS[key].view(np.uint32)), key
    # the key alone changes nothing of a plain fit; an explicit number wins and the estimate is still reported
    plain, est = run(brain), run(brain, doEstimateNoise='MPPCA', noise_patch=3)
    assert np.array_equal(est.RESULTS['MAPs'], plain.RESULTS['MAPs']) and set(est.RESULTS) - set(plain.RESULTS) == {'NOISE_MAPs'}
    assert est.get_config('noise_sigma_estimated') == sigma and plain.get_config('noise_method') is None
    est.set_config('doEstimateNoise', False)                     # the same Evaluation once more without the key: nothing lingers
    est.set_data(brain['img'], brain['sch'], brain['mask'])
    est.fit()
    assert est.get_config('noise_method') is None and 'NOISE_MAPs' not in est.RESULTS
    on = run(brain, doEstimateNoise='MPPCA', noise_patch=3, doDebiasSignal=True, DWI_SNR=17.0)
    off = run(brain, doDebiasSignal=True, DWI_SNR=17.0)
    assert np.array_equal(on.RESULTS['MAPs'], off.RESULTS['MAPs']) and on.get_config('DWI-SNR_estimated') == snr != 17.0


def test_evaluation_no_eligible_voxel_is_the_existing_error(brain):
    import amico_amd
    ae = amico_amd.Evaluation()
    ae.set_config('doEstimateNoise', 'MPPCA')
    mask = np.zeros_like(brain['mask'])
    mask[::3, ::3, ::3] = 1                                       # no cube holds half of its voxels
    ae.set_data(brain['img'], brain['sch'], mask)
    ae.set_model('NODDI')
    ae.set_kernels(brain['K'], brain['ht'])
    with pytest.raises(RuntimeError, match='doEstimateNoise: no voxel of the mask has a patch'):
        ae.fit()
