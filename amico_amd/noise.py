"""The noise level of an image from the spread of its b0 repeats (`Evaluation`'s key doEstimateNoise).

Per voxel the mean m and the sample standard deviation sd (ddof = 1) of the k b0 samples (`amx_noise_b0_*`, include/amico_amd.h, which
fixes the arithmetic); over the eligible voxels

    SNR_est   = nanmedian(m / sd) * sqrt(m_nu)
    sigma_est = nanmedian(sd)     / sqrt(m_nu)              nu = k - 1,  m_nu = median of a chi-square_nu variable over its mean

With Gaussian noise of one SNR for the whole image (sigma_v = b0_v / SNR: the reference's own noise model, preproc.py:30-34)
sd^2 nu / sigma^2 is chi-square_nu, and the median commutes with monotone maps: both estimates are median-unbiased for every k >= 2.
The magnitude image's noise is Rician; at b0 SNR >= 10 the Gaussian statement holds to better than 1 %.
Both medians are exact and taken on the GPU (`amx_nanmedian_device`).  There is no CPU fallback.
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
