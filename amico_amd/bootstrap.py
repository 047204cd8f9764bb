"""Wild (residual) bootstrap of a fit's maps on the GPU: B refits per voxel -> a per-voxel mean and standard error.

A replicate is the fitted signal plus the fit's residual with a random sign per sample,
    y_b = max(0, y_est + s * (y - y_est)),    s = +-1 (Rademacher; include/amico_amd.h has the counter-based generator)
fitted by the model's own `amx_<model>_fit_device[_f32]` -- the kernels of the original fit -- with the ORIGINAL fit's directions: the
tensor fit is not repeated, so the uncertainty is conditional on the direction.  Every row is resampled, the b0 rows included.  The
maps of the replicates are folded into Welford's running moments in fp64; nothing but the final mean and std leaves the loop.
"""
from . import _capi

MAX_SAMPLES = 10000
REFUSE_SANDI = ('the wild bootstrap is not built for SANDI: the only prediction the library has for it is the reference\'s quirk (rescaled '
                'coefficients on the normalised dictionary), which is not a prediction of y, so its residuals mean nothing')


def _as_int(value):
    import operator
    if isinstance(value, bool):
        return None
    try:
        return operator.index(value)
    except TypeError:
        return None


def check_samples(samples):
    """`samples` (bootstrap_samples) as an int in 2 .. 10 000, or ValueError"""
    b = _as_int(samples)
    if b is None or not 2 <= b <= MAX_SAMPLES:
        raise ValueError(f'bootstrap_samples must be an integer in 2 .. {MAX_SAMPLES}, not {samples!r}')
    return b


def check_seed(seed):
    s = _as_int(seed)
    if s is None or not 0 <= s < 2 ** 64:
        raise ValueError(f'bootstrap_seed must be an integer in 0 .. 2^64 - 1, not {seed!r}')
    return s


def config(evaluation):
    """(samples, seed) of an Evaluation whose 'bootstrap_samples' is set (None or 0: off -> None); 'bootstrap_seed' defaults to 0"""
    samples = evaluation.get_config('bootstrap_samples')
    if samples is None or samples is False or (not isinstance(samples, str) and samples == 0):
        return None
    seed = evaluation.get_config('bootstrap_seed')
    return check_samples(samples), check_seed(0 if seed is None else seed)


def wild_bootstrap(ctx, row, lut, y_t, dirs_t, lambda1, lambda2, extras, x_t, samples, seed=0, first_voxel=0, stream=None):
    """(mean_t, std_t), float64 device tensors [n_vox, n_maps]: mean and standard deviation (ddof = 1) of the maps over `samples`
    wild-bootstrap refits.  row: the model's _capi.FIT row; lut, y_t (f32 | f64), dirs_t, lambda1, lambda2, extras: what the original
    fit was called with; x_t: the coefficients that fit left (return_x=True; NODDI's [n, 3, n_atoms] layout is taken as it is);
    seed, first_voxel: the signs of voxel i are those of voxel first_voxel + i of a call that starts at 0.
    Everything is enqueued on `stream` with no host synchronisation in between and nothing allocated per replicate: one replicate
    buffer, one maps buffer, the two moments.  The caller synchronises (ctx.sync(stream)).  A progress callback registered on the
    context sees the ticks of every replicate's fit."""
    import torch
    samples, seed = check_samples(samples), check_seed(seed)
    if row.stem == 'sandi':
        raise NotImplementedError(REFUSE_SANDI)
    y_est = _capi.predict_device(ctx, lut, x_t, dirs_t, stream=stream)
    n = y_t.shape[0]
    width = row.outputs[0].shape(lut, extras)
    f64 = dict(dtype=torch.float64, device=y_t.device)
    y_b = torch.empty_like(y_t)
    est, mean, m2 = (torch.empty((n,) + width, **f64) for _ in range(3))
    for b in range(samples):
        _capi.bootstrap_resample_device(ctx, y_t, y_est, seed, b, first_voxel, stream, into=y_b)
        _capi._fit_device(row, ctx, lut, y_b, dirs_t, lambda1, lambda2, extras, {}, stream, False, False, into=est)
        _capi.bootstrap_accumulate_device(ctx, est, b + 1, mean, m2, stream)
    std = _capi.bootstrap_std_device(ctx, m2, samples, stream)
    return mean, std
