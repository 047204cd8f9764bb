"""The noise level of an image from the spread of its b0 repeats (`Evaluation`'s key doEstimateNoise).

Per voxel the mean m and the sample standard deviation sd (ddof = 1) of the k b0 samples (`amx_noise_b0_*`, include/amico_amd.h, which
fixes the arithmetic); over the eligible voxels

    SNR_est   = nanmedian(m / sd) * sqrt(m_nu)
    sigma_est = nanmedian(sd)     / sqrt(m_nu)              nu = k - 1,  m_nu = median of a chi-square_nu variable over its mean

With Gaussian noise of one SNR for the whole image (sigma_v = b0_v / SNR: the reference's own noise model, preproc.py:30-34)
sd^2 nu / sigma^2 is chi-square_nu, and the median commutes with monotone maps: both estimates are median-unbiased for every k >= 2.
The magnitude image's noise is Rician; at b0 SNR >= 10 the Gaussian statement holds to better than 1 %.
Both medians are exact and taken on the GPU (`amx_nanmedian_device`).  There is no CPU fallback.

A second estimator needs no b0 repeat (doEstimateNoise = 'MPPCA'): `estimate_mppca_device` / `estimate_mppca` take a sigma per voxel
from the Marchenko-Pastur edge of the eigenvalues of its local patch over all volumes (`amx_prep_noise_mppca_device`), and the same two medians.
`denoise_mppca_device` / `denoise_mppca` go on from there to the denoised image (`Evaluation`'s key doDenoise): every eligible
voxel becomes the centre column of its patch's best approximation of rank n_signal (`amx_prep_noise_mppca_denoise_device`).
"""
import numpy as np
from scipy import special

from . import _capi

MIN_B0, MAX_B0 = 2, 128       # b0 volumes the estimate takes (include/amico_amd.h)


def chi2_median_ratio(nu):
    """m_nu = 2 gammaincinv(nu / 2, 1 / 2) / nu: the median of a chi-square variable of nu degrees of freedom over its mean
    (m_1 = 0.45494, m_2 = ln 2, m_9 = 0.92698)"""
    nu = float(nu)
    if not nu > 0:
        raise ValueError('nu must be > 0')
    return float(2.0 * special.gammaincinv(0.5 * nu, 0.5) / nu)


def check_b0_count(k):
    """the sentence Evaluation.set_data raises for a scheme the estimate cannot take"""
    if k < MIN_B0 or k > MAX_B0:
        raise RuntimeError(f'doEstimateNoise: the noise level is estimated from the spread of the b0 repeats and needs {MIN_B0} to {MAX_B0} '
                           f'b0 volumes; the scheme has {k}')


def _finish(k, words):
    """words f64 [6] as the two medians left them: ratio's (lower, upper), sd's (lower, upper), then the two counts as int64 bits
    (one number: an ineligible voxel is NaN in both vectors)"""
    c = int(words[4:6].view(np.int64)[0])
    if c == 0:
        return float('nan'), float('nan'), 0
    root = np.sqrt(chi2_median_ratio(k - 1))
    with np.errstate(over='ignore'):
        snr = float((words[0] + words[1]) / 2.0 * root)           # numpy's nanmedian: the mean of the two middle values
        sigma = float((words[2] + words[3]) / 2.0 / root)
    return snr, sigma, c


def _medians(ctx, t_ratio, t_sd, words, stream=None):
    """the two medians into `words` (a float64 device tensor [6], the layout _finish reads); nothing waits"""
    n = t_ratio.numel()
    base = words.data_ptr()
    _capi.nanmedian_device(ctx, t_ratio.data_ptr(), n, base, base + 32, stream)
    _capi.nanmedian_device(ctx, t_sd.data_ptr(), n, base + 16, base + 40, stream)


def estimate_device(plan, d_img, stream=None):
    """plan: a `_capi.Prep`; d_img: device pointer (int) of the float32 image's element buffer in the plan's layout.
    -> {'snr', 'sigma', 'voxels', 'mean', 'sd'}: the two estimates (NaN when no voxel is eligible), the number of eligible voxels, and
    the per-voxel b0 mean and standard deviation as float64 device tensors [n_vox] in the plan's masked order (NaN where not eligible).
    One k_noise_b0 launch, two medians, one small copy home."""
    import torch
    check_b0_count(plan.n_b0)
    dev = torch.device('cuda', torch.cuda.current_device())
    buf = torch.empty((3, plan.n_vox), dtype=torch.float64, device=dev)
    words = torch.empty(6, dtype=torch.float64, device=dev)
    plan.noise_b0_device(d_img, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), stream)
    _medians(plan.ctx, buf[2], buf[1], words, stream)
    snr, sigma, c = _finish(plan.n_b0, words.cpu().numpy())            # (the copy on the null stream waits for the kernels)
    return {'snr': snr, 'sigma': sigma, 'voxels': c, 'mean': buf[0], 'sd': buf[1]}


MPPCA = 'MPPCA'               # the value of doEstimateNoise that selects the estimator below (any letter case)
MPPCA_PATCHES = (3, 5)


def is_mppca(value):
    """doEstimateNoise names the Marchenko-Pastur estimator"""
    return isinstance(value, str) and value.upper() == MPPCA


def check_patch(patch):
    """noise_patch: 3 or 5 (ValueError otherwise), as an int"""
    if isinstance(patch, bool) or not isinstance(patch, (int, np.integer)) or int(patch) not in MPPCA_PATCHES:
        raise ValueError('noise_patch (the edge of the Marchenko-Pastur patch) must be 3 or 5, got %r' % (patch,))
    return int(patch)


def check_patch_fits(shape3, patch):
    """the sentence Evaluation.set_data raises for a volume the patch does not fit into"""
    if min(int(d) for d in shape3) < patch:
        raise RuntimeError(f"doEstimateNoise: 'MPPCA' with noise_patch {patch} needs a volume of at least {patch} voxels along every axis; "
                           f'the image is {tuple(int(d) for d in shape3)}')


def estimate_mppca_device(plan, d_img, patch=5, stream=None):
    """The noise level per voxel by Marchenko-Pastur PCA of its patch of edge `patch` (include/amico_amd.h fixes the arithmetic).
    plan: a `_capi.Prep`; d_img: device pointer (int) of the float32 image's element buffer in the plan's layout.
    -> {'snr', 'sigma', 'voxels', 'mean', 'sd', 'signal'}: nanmedian(mean / sigma) (NaN without a b0 volume) and nanmedian(sigma) over the
    eligible voxels (no chi-square factor: sigma is no sample standard deviation), their number, and per voxel the b0 mean, sigma (under
    'sd', the key the b0 estimator's callers read) and the number of signal components as float64 device tensors [n_vox] in the plan's
    masked order, NaN where not eligible.  One k_mppca launch, two medians, one small copy home.  On small patches sigma is a few percent
    low (its finite-size property); the Rician caveat of the b0 estimator holds here as well."""
    import torch
    patch = check_patch(patch)
    dev = torch.device('cuda', torch.cuda.current_device())
    buf = torch.empty((4, plan.n_vox), dtype=torch.float64, device=dev)          # sigma, signal components, mean, ratio
    plan.noise_mppca_device(d_img, patch, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), None, stream)
    return _mppca_result(plan, buf, stream)


def _mppca_result(plan, buf, stream=None):
    """buf f64 [4, n_vox] as a Marchenko-Pastur launch left it (sigma, signal components, mean, ratio) -> the dict of
    `estimate_mppca_device`: two medians, one small copy home"""
    import torch
    words = torch.empty(6, dtype=torch.float64, device=buf.device)
    base = words.data_ptr()
    _capi.nanmedian_device(plan.ctx, buf[3].data_ptr(), plan.n_vox, base, base + 32, stream)           # ratio: count in word 4
    _capi.nanmedian_device(plan.ctx, buf[0].data_ptr(), plan.n_vox, base + 16, base + 40, stream)      # sigma: count in word 5
    w = words.cpu().numpy()                                                      # (the copy on the null stream waits for the kernels)
    c_ratio, c_sigma = (int(v) for v in w[4:6].view(np.int64))
    with np.errstate(over='ignore'):
        snr = float((w[0] + w[1]) / 2.0) if c_ratio else float('nan')
        sigma = float((w[2] + w[3]) / 2.0) if c_sigma else float('nan')
    return {'snr': snr, 'sigma': sigma, 'voxels': c_sigma, 'mean': buf[2], 'sd': buf[0], 'signal': buf[1]}


def estimate_mppca(img, mask, b0_idx, patch=5, ctx=None):
    """img float32 [X, Y, Z, nS] (numpy, C or Fortran order; anything else is copied to C-order float32), mask [X, Y, Z] (voxels == 1 are
    taken; None: all), b0_idx: the b0 volumes (may be empty) -> the dict of `estimate_mppca_device` with 'mean' / 'sd' / 'signal' as float64
    numpy [n_vox] in the mask's C order.  Uploads, one wait, numpy out."""
    import torch
    from .models import get_context
    patch = check_patch(patch)
    img = np.asarray(img)
    if img.ndim != 4:
        raise ValueError('img must be [X, Y, Z, nS]')
    if img.dtype != np.float32 or not (img.flags.c_contiguous or img.flags.f_contiguous):
        img = np.ascontiguousarray(img, dtype=np.float32)
    sel = np.ones(img.shape[:3], dtype=bool) if mask is None else np.asarray(mask) == 1
    if sel.shape != img.shape[:3]:
        raise ValueError('mask geometry does not match the image')
    check_patch_fits(img.shape[:3], patch)
    rank = np.full(sel.shape, -1, dtype=np.int32)
    rank[sel] = np.arange(int(sel.sum()), dtype=np.int32)
    ctx = ctx if ctx is not None else get_context()
    plan = _capi.Prep(ctx, img.shape, tuple(s // 4 for s in img.strides), rank, [[i] for i in range(img.shape[3])],
                      np.asarray(b0_idx, dtype=np.int32).ravel())
    try:
        dev = torch.device('cuda', torch.cuda.current_device())
        d_img = torch.from_numpy(plan._img_buffer(img)).to(dev)
        res = estimate_mppca_device(plan, d_img.data_ptr(), patch)
        for k in ('mean', 'sd', 'signal'):
            res[k] = res[k].cpu().numpy()
    finally:
        plan.close()
    return res


DENOISE_STATUS = ('denoised', 'not eligible', 'over the cap')      # d_status of amx_prep_noise_mppca_denoise_device


def is_denoise(value):
    """doDenoise: 'MPPCA' in any letter case or True -> True; False / None -> False; anything else is a ValueError"""
    if value is None or value is False:
        return False
    if value is True or is_mppca(value):
        return True
    raise ValueError("doDenoise must be 'MPPCA', True or False, got %r" % (value,))


def denoise_mppca_device(plan, d_img, patch=5, stream=None):
    """The image denoised by Marchenko-Pastur PCA of local patches (include/amico_amd.h fixes the arithmetic): every eligible
    voxel of the mask gets the centre column of its patch's best approximation of rank n_signal; every other sample is the image's.
    plan: a `_capi.Prep`; d_img: device pointer (int) of the float32 image's element buffer in the plan's layout (left as it is).
    -> the dict of `estimate_mppca_device` -- the same bits: the launch delivers the estimate as well -- and 'image': a float32 device
    tensor of plan.extent elements in the image's layout; 'status': int32 device tensor [n_vox] (the index into DENOISE_STATUS);
    'denoised' / 'passed_through': the number of voxels with status 0 / any other.  One k_mppca_denoise launch behind a device copy,
    two medians, two small copies home."""
    import torch
    patch = check_patch(patch)
    dev = torch.device('cuda', torch.cuda.current_device())
    buf = torch.empty((4, plan.n_vox), dtype=torch.float64, device=dev)
    out = torch.empty(plan.extent, dtype=torch.float32, device=dev)
    status = torch.empty(plan.n_vox, dtype=torch.int32, device=dev)
    plan.noise_mppca_denoise_device(d_img, patch, out.data_ptr(), buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(),
                                    status.data_ptr(), None, stream)
    res = _mppca_result(plan, buf, stream)
    done = int((status == 0).sum().item())
    res.update(image=out, status=status, denoised=done, passed_through=plan.n_vox - done)
    return res


def denoise_mppca(img, mask, b0_idx, patch=5, ctx=None):
    """img, mask, b0_idx as `estimate_mppca` takes them -> its dict and 'image': float32 numpy of img's shape and memory order, 'status':
    int32 numpy [n_vox] in the mask's C order, 'denoised', 'passed_through'.  Uploads, one wait, numpy out."""
    import torch
    from .models import get_context
    patch = check_patch(patch)
    img = np.asarray(img)
    if img.ndim != 4:
        raise ValueError('img must be [X, Y, Z, nS]')
    if img.dtype != np.float32 or not (img.flags.c_contiguous or img.flags.f_contiguous):
        img = np.ascontiguousarray(img, dtype=np.float32)
    sel = np.ones(img.shape[:3], dtype=bool) if mask is None else np.asarray(mask) == 1
    if sel.shape != img.shape[:3]:
        raise ValueError('mask geometry does not match the image')
    check_patch_fits(img.shape[:3], patch)
    rank = np.full(sel.shape, -1, dtype=np.int32)
    rank[sel] = np.arange(int(sel.sum()), dtype=np.int32)
    ctx = ctx if ctx is not None else get_context()
    plan = _capi.Prep(ctx, img.shape, tuple(s // 4 for s in img.strides), rank, [[i] for i in range(img.shape[3])],
                      np.asarray(b0_idx, dtype=np.int32).ravel())
    try:
        dev = torch.device('cuda', torch.cuda.current_device())
        d_img = torch.from_numpy(plan._img_buffer(img)).to(dev)
        res = denoise_mppca_device(plan, d_img.data_ptr(), patch)
        for k in ('mean', 'sd', 'signal', 'status'):
            res[k] = res[k].cpu().numpy()
        res['image'] = np.lib.stride_tricks.as_strided(res['image'].cpu().numpy(), shape=img.shape, strides=img.strides)
    finally:
        plan.close()
    return res


def estimate_from_rows(y, b0_idx, ctx=None):
    """y f32 | f64 [n, nS] (numpy; any other dtype is taken as float64), b0_idx: the columns of the b0 repeats, 2 to 128 of them.
    -> {'snr', 'sigma', 'voxels', 'mean', 'sd'}: 'mean' / 'sd' float64 numpy [n], NaN where a row is not eligible (a sample that is
    not finite, a mean <= 0, no spread).  Uploads, one wait, numpy out."""
    import torch
    from .models import get_context
    y = np.asarray(y)
    if y.ndim != 2:
        raise ValueError('y must be [n, nS]')
    f32 = y.dtype == np.float32
    y = np.ascontiguousarray(y, dtype=np.float32 if f32 else np.float64)
    b0 = np.ascontiguousarray(b0_idx, dtype=np.int32).ravel()
    ctx = ctx if ctx is not None else get_context()
    n, nS = y.shape
    dev = torch.device('cuda', torch.cuda.current_device())
    d_y = torch.from_numpy(y).to(dev)
    buf = torch.empty(3 * n + 6, dtype=torch.float64, device=dev)      # mean, sd, the medians' six words, ratio: the first three go home
    mean, sd, words, ratio = buf[:n], buf[n:2 * n], buf[2 * n:2 * n + 6], buf[2 * n + 6:]
    _capi.noise_b0_rows_device(ctx, d_y.data_ptr(), n, nS, b0, mean.data_ptr(), sd.data_ptr(), ratio.data_ptr(), f32=f32)
    _medians(ctx, ratio, sd, words)
    host = buf[:2 * n + 6].cpu().numpy()
    snr, sigma, c = _finish(len(b0), host[2 * n:])
    return {'snr': snr, 'sigma': sigma, 'voxels': c, 'mean': host[:n], 'sd': host[n:2 * n]}
