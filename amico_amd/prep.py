"""Signal preparation around the fit (SURVEY section 8 f, rows 2-3), host side.

What `Evaluation.load_data` does to the 4-D image after reading it (core.py:209-268) and what `Evaluation.fit`
does to get `y` (core.py:451-452) and to store the results (core.py:472-498), with the optional Rician debias in front
(core.py:201-206 -> preproc.py:23-36), planned once per (image geometry,
mask, scheme, options) and executed on the GPU through `amx_prep_*` (include/amico_amd.h).  No CPU fallback.
"""
import numbers
import warnings

import numpy as np

from . import _capi

MAX_DEBIAS_B0 = 128      # b0 volumes the debias kernel sums in numpy's order (include/amico_amd.h)

# the reference's sentences (core.py:155, 158, 273, 276), with set_data() in place of load_data()
BAD_RAW = 'Nan or Inf values in the raw signal.'
BAD_PREPROCESSED = 'Nan or Inf values in the signal after the pre-processing.'
_BAD_TRY = ' Try using the "replace_bad_voxels" or "b0_min_signal" parameters when calling "set_data()"'


def check_replace_bad_voxels(value):
    """load_data's `replace_bad_voxels` (core.py:122-123): None, or the number that takes the place of NaN / Inf samples.
    -> the value as given.  The image is float32: a value that is not finite AS A FLOAT32 would plant the very thing it is meant
    to remove, so it is refused here -- on the host, before any context exists -- like a value that is no number at all."""
    if value is None:
        return None
    if not isinstance(value, (numbers.Real, np.integer, np.floating)):
        raise ValueError(f'replace_bad_voxels must be None or a finite number, not {value!r}')
    try:
        with np.errstate(over='ignore'):
            finite = bool(np.isfinite(np.float32(value)))
    except OverflowError:
        finite = False
    if not finite:
        raise ValueError(f'replace_bad_voxels must be finite as a float32, not {value!r}')
    return value


def check_scaling(scaling):
    """The NIfTI header's (scl_slope, scl_inter) as set_data takes it -> (slope, inter) as floats, or None for "no scaling": None,
    a pair whose slope is None (what nibabel reports for an unscaled image) or the identity (1, 0).  A missing intercept is 0.
    A value that is not finite, or a zero slope, is refused here -- on the host, before any context exists."""
    if scaling is None:
        return None
    try:
        slope, inter = scaling
    except (TypeError, ValueError):
        raise ValueError(f'scaling must be None or the pair (slope, inter), not {scaling!r}') from None
    if slope is None:
        return None
    inter = 0.0 if inter is None else inter
    for name, v in (('slope', slope), ('inter', inter)):
        if not isinstance(v, (numbers.Real, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f'scaling: {name} must be a finite number, not {v!r}')
    if slope == 0:
        raise ValueError('scaling: slope must not be 0')
    slope, inter = float(slope), float(inter)
    return None if (slope == 1.0 and inter == 0.0) else (slope, inter)


def to_float32(raw, scaling=None):
    """core.py:136 on the host, the statement the ingest kernel is held to: np.float32(raw), or with the header's scaling
    np.float32(np.float64(raw) * slope + inter) -- nibabel's scaling in float64, then the cast.  `scaling` as check_scaling returns it."""
    raw = np.asarray(raw)
    with np.errstate(over='ignore', invalid='ignore'):
        if scaling is None:
            return raw.astype(np.float32, copy=False)
        return (raw.astype(np.float64) * scaling[0] + scaling[1]).astype(np.float32)


def streamable(raw):
    """can the image cross the link as it is stored?  One of the six dtypes amx_prep_ingest converts, and a layout that is a
    permutation of a contiguous block (C order, nibabel's Fortran order)"""
    if raw.dtype not in _capi.RAW_DTYPES or raw.ndim != 4 or raw.size == 0:
        return False
    if any(st <= 0 or st % raw.itemsize for st in raw.strides):
        return False
    expect = raw.itemsize
    for st, d in sorted((st, d) for st, d in zip(raw.strides, raw.shape) if d != 1):
        if st != expect:
            return False
        expect *= d
    return True


def refuse_or_warn(count, replace, sentence):
    """core.py:153-158 / 271-276 once the scan has counted `count` bad samples: nothing to do, a warning, or the refusal"""
    if count == 0:
        return
    if replace is None:
        raise RuntimeError(sentence + _BAD_TRY)
    warnings.warn(f'{sentence} They will be replaced with: {replace}')


def volume_groups(scheme, do_merge_b0=False, do_directional_average=False):
    """output volume -> input volumes whose float32 mean it is.
    plain: identity; doMergeB0 (core.py:225-227): [b0 volumes] + each DWI volume;
    doDirectionalAverage (core.py:229-252): [b0 volumes] + one group per shell, shells sorted by b-value."""
    b0 = [int(i) for i in scheme.b0_idx]
    if do_directional_average:
        shells = scheme.shells
        order = np.argsort([sh['b'] for sh in shells])
        return [b0] + [[int(i) for i in shells[k]['idx']] for k in order]
    if do_merge_b0:
        return [b0] + [[int(i)] for i in scheme.dwi_idx]
    return [[i] for i in range(scheme.nS)]


def directional_average_table(scheme):
    """the 7-column scheme table of the shell-averaged data (core.py:232-252): b0 row + one x-gradient per shell"""
    shells = scheme.shells
    order = np.argsort([sh['b'] for sh in shells])
    rows = [[1, 0, 0, 0, 0, 0, 0]]
    for k in order:
        sh = shells[k]
        rows.append([1, 0, 0, sh['G'], sh['Delta'], sh['delta'], sh['TE']])
    return np.array(rows, dtype=np.float64)


class SignalPreparation:
    """image [X, Y, Z, nS] float32 (any strides) + mask -> y f64[n_vox, n_out]; per-voxel results -> volumes.
    The image may also be given as it is stored (uint8 / int16 / uint16 / int32 / float64, or float32 with a scaling) in a streamable
    layout: the plan is made on its shape and element strides and the float32 image is made on the GPU (amx_prep_ingest)."""

    def __init__(self, scheme, img_like, mask, do_normalize=True, do_merge_b0=False, do_directional_average=False,
                 b0_min_signal=0.0, ctx=None, debias_snr=None, replace_bad_voxels=None, scaling=None):
        """debias_snr (DWI-SNR, or None = doDebiasSignal off): the image is debiased first, on the voxels with mask != 0
        (preproc.py:29), and is zero elsewhere (preproc.py:24).
        replace_bad_voxels (core.py:122-123; None = no scan at all): gather() replaces the NaN / Inf samples of a private copy of
        the image before anything else reads it (core.py:152-156) and those of y after the gather (core.py:270-274, on the masked
        voxels' rows); the counts are left in bad_samples_raw / bad_samples_preprocessed and a warning is raised when one is not 0"""
        from .models import get_context
        self.replace_bad_voxels = check_replace_bad_voxels(replace_bad_voxels)      # (before a context is made)
        self.scaling = check_scaling(scaling)
        self.bad_samples_raw = self.bad_samples_preprocessed = None
        self.raw = img_like.dtype != np.float32 or self.scaling is not None       # the float32 image is made by the ingest kernel
        if img_like.ndim != 4 or (img_like.dtype != np.float32 and not streamable(img_like)):
            raise ValueError('DWI image must be a 4D float32 array')
        if self.raw and not streamable(img_like):
            raise ValueError('an image with a scaling must have a streamable layout (C or Fortran order)')
        isz = img_like.itemsize
        if img_like.shape[3] != scheme.nS:
            raise ValueError('Scheme does not match with DWI data')                     # core.py:177-178
        if mask.shape != img_like.shape[:3]:
            raise ValueError('MASK geometry does not match with DWI data')              # core.py:191-192
        if any(s % isz or s <= 0 for s in img_like.strides):
            raise ValueError('image strides must be positive multiples of the element size')
        if do_normalize and scheme.b0_count == 0:
            raise RuntimeError('No b0 volume to normalize signal with')                 # core.py:214-215
        if debias_snr is not None and scheme.b0_count == 0:
            raise RuntimeError('No b0 volume to estimate the noise level from (doDebiasSignal)')   # preproc.py:30-31: sigma = mean(b0) / SNR
        if debias_snr is not None and scheme.b0_count > MAX_DEBIAS_B0:
            raise RuntimeError(f'doDebiasSignal: more than {MAX_DEBIAS_B0} b0 volumes are not supported')
        self.debias_snr = None if debias_snr is None else float(debias_snr)
        self.scheme = scheme
        self.do_normalize = bool(do_normalize)
        self.b0_min_signal = float(b0_min_signal)
        self.groups = volume_groups(scheme, do_merge_b0, do_directional_average)
        self.sel = np.asarray(mask) == 1                                                # core.py:451: == 1, not != 0
        rank = np.full(self.sel.shape, -1, dtype=np.int32)
        rank[self.sel] = np.arange(int(self.sel.sum()), dtype=np.int32)                 # C-order enumeration
        self.ctx = ctx if ctx is not None else get_context()
        self._plan = _capi.Prep(self.ctx, img_like.shape, tuple(s // isz for s in img_like.strides), rank, self.groups,
                                scheme.b0_idx, overwrite_in_order=bool(do_directional_average))
        self.n_vox, self.n_out = self._plan.n_vox, self._plan.n_out
        self.mean_b0s = None
        if self.debias_snr is not None:
            self._plan.set_debias_mask(mask)

    def debias(self, img):
        """-> the debiased float32 image (a copy in the same layout; `img` itself when debias_snr is None)"""
        if self.debias_snr is None:
            return img
        out = np.lib.stride_tricks.as_strided(np.array(self._plan._img_buffer(img)), shape=img.shape, strides=img.strides)
        return self._plan.debias(out, self.debias_snr)

    def b0_threshold(self, img):
        """right-hand side of core.py:217; needs the b0 mean of every voxel only when b0_min_signal != 0"""
        if not self.do_normalize or self.b0_min_signal == 0.0:
            return np.float32(0.0)
        mean_b0s = self._plan.mean_b0(img)                                               # (of the debiased image: zero outside its mask)
        return self.b0_min_signal * mean_b0s[mean_b0s > 0].mean()

    def gather(self, img):
        """-> (y f64[n_vox, n_out], mean_b0 f32[n_vox] of the masked voxels or None)"""
        r = self.replace_bad_voxels
        if self.raw:
            # the stored image -> float32, scanned (and replaced) by the same kernel: core.py:136 + 152-156
            img, bad = self._plan.ingest(img, self.scaling, r)
            if r is not None:
                self.bad_samples_raw = bad
                refuse_or_warn(bad, r, BAD_RAW)
        elif r is not None:
            img = np.lib.stride_tricks.as_strided(np.array(self._plan._img_buffer(img)), shape=img.shape, strides=img.strides)
            self.bad_samples_raw = self._plan.sanitize(img, r)                          # core.py:152-156
            refuse_or_warn(self.bad_samples_raw, r, BAD_RAW)
        img = self.debias(img)
        y, mb0 = self._plan.gather(img, self.do_normalize, float(self.b0_threshold(img)))
        if r is not None:
            self.bad_samples_preprocessed = _capi.sanitize(self.ctx, y, r)              # core.py:270-274
            refuse_or_warn(self.bad_samples_preprocessed, r, BAD_PREPROCESSED)
        self.mean_b0s = mb0
        return y, mb0

    def scatter(self, values):
        """per-voxel values [n_vox(, k)] -> float32 volume [X, Y, Z(, k)], zero outside the mask (core.py:472-498)"""
        vol = self._plan.scatter(values)
        return vol[..., 0] if np.ndim(values) == 1 else vol
