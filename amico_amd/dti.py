"""Principal fibre directions from the log-linear diffusion-tensor fit (SURVEY section 8 f, row 1).

Mirrors what `Evaluation.fit` does before `model.fit` (core.py:431-436, 456-458):

    gtab = gradient_table(bvals=scheme.b, bvecs=scheme.raw[:, :3])
    DTI  = dti.TensorModel(gtab, fit_method='OLS')
    DIRs = np.squeeze(DTI.fit(y).directions)

and the same with `fit_method` 'WLS' or 'NLLS' (the configuration's DTI_fit_method, core.py:419-420, 436), and with 'RT' | 'RESTORE'
| 'restore' once a noise level `sigma` is given (the reference's call passes none, so dipy raises there).

The one-off part (gradient table, design matrix, pseudo-inverse: a 7 x nS matrix per scheme) is host numpy,
like the reference; the per-voxel part (log, contraction, 3x3 eigen-decomposition) runs on the GPU through
`amx_dti_directions*` (include/amico_amd.h).  There is no CPU fallback.

The same fit also gives what a study reports beside the model's maps -- `TensorFit.evals`, `.fa`, `.md`, `.ad`, `.rd` -- through
`amx_dti_fit*`: `TensorDirections.fit_maps`, and `Evaluation`'s config key `doSaveTensorMaps`.
"""
import numpy as np

from . import _capi

MIN_POSITIVE_SIGNAL = 1e-4      # dipy.reconst.dti.MIN_POSITIVE_SIGNAL (TensorModel.fit default)
MIN_DIFFUSIVITY_TOL = 1e-6      # TensorModel.__init__: min_diffusivity = tol / -design_matrix.min()
SCALAR_NAMES = ('FA', 'MD', 'AD', 'RD')     # the columns of `scalars`


def gradient_table(bvals, bvecs, b0_threshold=50.0, atol=1e-2):
    """(bvals, bvecs) as dipy.core.gradients.gradient_table_from_bvals_bvecs + GradientTable see them: vectors
    that are not unit length are only legal on b0 volumes, where they (and the b-value) are zeroed; the table
    then carries bvals = |b g| and bvecs = b g / |b g|."""
    bvals = np.asarray(bvals, dtype=np.float64)
    bvecs = np.asarray(bvecs, dtype=np.float64)
    if bvecs.shape != (bvals.shape[0], 3):
        raise ValueError('bvecs must be [nS, 3]')
    bvecs = np.where(np.isnan(bvecs), 0.0, bvecs)
    unit = np.abs(np.sqrt((bvecs * bvecs).sum(1)) - 1.0) <= atol
    if not np.all(unit[bvals > b0_threshold]):
        raise ValueError('The vectors in bvecs should be unit')
    bvecs = np.where(unit[:, None], bvecs, 0.0)
    grads = (bvals * unit)[:, None] * bvecs
    b = np.sqrt((grads * grads).sum(1))
    g = np.zeros_like(grads)
    nz = b > 0
    g[nz] = grads[nz] / b[nz, None]
    return b, g


def design_matrix(bvals, bvecs):
    """dipy.reconst.dti.design_matrix: rows -[b gx^2, 2 b gx gy, b gy^2, 2 b gx gz, 2 b gy gz, b gz^2, 1]."""
    B = np.zeros((bvals.shape[0], 7))
    B[:, 0] = bvecs[:, 0] * bvecs[:, 0] * bvals
    B[:, 1] = bvecs[:, 0] * bvecs[:, 1] * 2.0 * bvals
    B[:, 2] = bvecs[:, 1] * bvecs[:, 1] * bvals
    B[:, 3] = bvecs[:, 0] * bvecs[:, 2] * 2.0 * bvals
    B[:, 4] = bvecs[:, 1] * bvecs[:, 2] * 2.0 * bvals
    B[:, 5] = bvecs[:, 2] * bvecs[:, 2] * bvals
    B[:, 6] = 1.0
    return -B


FIT_METHODS = {'OLS': 'OLS', 'LS': 'OLS', 'WLS': 'WLS', 'NLLS': 'NLLS'}
ROBUST_METHODS = ('RT', 'RESTORE', 'restore')
# core.py:419-420 of the reference
FIT_METHOD_ERROR = ("DTI fit method must be one of the following:\n'OLS'(default) or 'LS': ordinary least squares\n"
                    "'WLS': weighted least squares\n'NLLS': non-linear least squares\n"
                    "'RT' or 'RESTORE' or 'restore': robust tensor\n"
                    "NOTE: more info at https://dipy.org/documentation/1.6.0./reference/dipy.reconst/#dipy.reconst.dti.TensorModel")


ROBUST_NEEDS_SIGMA = ("DTI_fit_method %r: the robust tensor fit needs a noise estimate (sigma), which the reference's own call "
                      "(TensorModel(gtab, fit_method=...)) does not pass either: it fails inside dipy.  Give one: sigma= to "
                      "TensorDirections; DTI_sigma, or DWI-SNR with doNormalizeSignal and a b0 volume, to Evaluation")


def resolve_sigma(fit_method, dti_sigma=None, snr=None, normalized=False):
    """The noise level Evaluation hands a robust fit, None for the other methods: DTI_sigma if set (ValueError unless a finite
    number > 0); else 1 / DWI-SNR when DWI-SNR is set and the signals are divided by their b0 mean (sigma = b0 / SNR there); else
    None, and TensorDirections raises its NotImplementedError where the tensor fit would run."""
    check_fit_method(fit_method)
    if fit_method not in ROBUST_METHODS:
        return None
    if dti_sigma is not None:
        return _capi.check_sigma(dti_sigma)
    if snr is not None and normalized:
        try:
            return _capi.check_sigma(1.0 / float(snr))
        except (TypeError, ValueError, ZeroDivisionError):
            raise ValueError('DWI-SNR must be a finite number > 0 to give the robust tensor fit its sigma, got %r' % (snr,))
    return None


def check_fit_method(name):
    """the reference's check of `DTI_fit_method` (core.py:419-420): ValueError for a name it does not know"""
    if name not in FIT_METHODS and name not in ROBUST_METHODS:
        raise ValueError(FIT_METHOD_ERROR)


class TensorDirections:
    """`TensorModel(gtab, fit_method=...).fit(y).directions` of the reference's call site, on the GPU.

    fit_method as the reference spells it: 'OLS' | 'LS' (log-linear least squares), 'WLS' (dipy's wls_fit_tensor: the
    log-linear fit weighted by the signal the OLS fit predicts), 'NLLS' (nlls_fit_tensor: the minimum of
    sum (s - exp(X p))^2 next to the linear fit), 'RT' | 'RESTORE' | 'restore' (restore_fit_tensor: NLLS, the samples more than
    3 sigma off a Geman-McClure fit left out, NLLS again without them; include/amico_amd.h says where it departs from dipy).

    sigma: the noise level of the robust fit, one finite number > 0 in the units of `y` (1 / SNR on signals divided by their b0).
    The reference's call never passes one and dipy raises for it there; here the robust names without a sigma are a
    NotImplementedError, and a sigma that is no finite positive number a ValueError.  With a merged-b0 table (`from_scheme(...,
    do_merge_b0=True)`) the one sigma applies to the merged b0 as well, although a mean of k volumes has sigma / sqrt(k): that is
    what dipy would do with the same table."""

    def __init__(self, bvals, bvecs, min_signal=None, ctx=None, fit_method='OLS', sigma=None):
        from .models import get_context
        check_fit_method(fit_method)
        if fit_method in ROBUST_METHODS:
            if sigma is None:
                raise NotImplementedError(ROBUST_NEEDS_SIGMA % (fit_method,))
            sigma = _capi.check_sigma(sigma)
        elif sigma is not None:
            raise ValueError('sigma belongs to the robust fit methods (%s)' % ', '.join(repr(m) for m in ROBUST_METHODS))
        if min_signal is not None and min_signal <= 0:
            raise ValueError('The `min_signal` key-word argument needs to be strictly positive.')   # dipy's check
        self.fit_method = 'RESTORE' if fit_method in ROBUST_METHODS else FIT_METHODS[fit_method]
        self.sigma = sigma
        self.bvals, self.bvecs = gradient_table(bvals, bvecs)
        self.design = design_matrix(self.bvals, self.bvecs)
        self.inv_design = np.linalg.pinv(self.design)
        self.min_signal = MIN_POSITIVE_SIGNAL if min_signal is None else float(min_signal)
        # TensorModel.__init__: the floor decompose_tensor clips the eigenvalues at (every entry of the design matrix is <= 0)
        self.min_diffusivity = MIN_DIFFUSIVITY_TOL / -self.design.min()
        self.ctx = ctx if ctx is not None else get_context()
        self._dti = _capi.Dti(self.ctx, self.inv_design, self.min_signal, design=self.design, method=self.fit_method, sigma=sigma)

    def last_unconverged(self):
        """NLLS, RESTORE: voxels of the last call that kept their starting (WLS) parameters, dipy's fallback; 0 otherwise"""
        return self._dti.last_unconverged()

    def last_robust(self):
        """RESTORE: of the last call, the voxels (that had a sample beyond 3 sigma and entered the reweighted fit, that were fitted
        anew without their outliers, whose reweighted fit reached its trip cap or gave up, that were left with fewer than 7
        inliers and kept the reweighted fit); zeros otherwise"""
        return self._dti.last_robust()

    @classmethod
    def from_scheme(cls, scheme, do_merge_b0=False, **kw):
        """core.py:428-432: with doMergeB0 the table is [one b0] + the DWI volumes."""
        b = np.asarray(scheme.b, dtype=np.float64)
        g = np.asarray(scheme.raw, dtype=np.float64)[:, :3]
        if do_merge_b0:
            idx = np.asarray(scheme.dwi_idx)
            b = np.hstack((0.0, b[idx]))
            g = np.vstack((np.zeros((1, 3)), g[idx]))
        return cls(b, g, **kw)

    def fit(self, y):
        """y [n_vox, nS] -> directions f64[n_vox, 3]."""
        return self._dti.directions(y)

    def fit_maps(self, y):
        """y [n_vox, nS] -> {'directions': f64[n_vox, 3], 'evals': f64[n_vox, 3], 'scalars': f64[n_vox, 4]}: the fit of `fit`, its
        eigenvalues in descending order clipped from below at `min_diffusivity` (dipy's decompose_tensor), and FA, MD, AD, RD
        (SCALAR_NAMES) of the clipped eigenvalues.  The directions are those of `fit`, bit for bit.  A NaN sample counts as
        min_signal, as every sample below min_signal does; a +Inf sample leaves NaN eigenvalues and scalars; an all-zero or
        constant voxel gives three times min_diffusivity and FA = 0 (include/amico_amd.h: amx_dti_fit).
        A robust estimator adds 'outliers': int32 [n_vox], the samples its 3-sigma verdict left out of the voxel's fit."""
        return self._dti.fit(y, self.min_diffusivity)

    def fit_device(self, d_y, n_vox, d_dirs, stream=None, f32=False, d_evals=None, d_scalars=None, d_outliers=None):
        """device pointers; d_evals f64 [n_vox, 3] / d_scalars f64 [n_vox, 4] (either may be None; d_dirs too when one of them is
        given).  Without them: the direction kernel of always, nothing else is launched.  d_outliers int32 [n_vox]: a robust
        estimator's outlier counts."""
        if d_evals is None and d_scalars is None and d_outliers is None:
            self._dti.directions_device(d_y, n_vox, d_dirs, stream, f32=f32)
        else:
            self._dti.fit_device(d_y, n_vox, self.min_diffusivity, d_dirs, d_evals, d_scalars, stream, f32=f32, d_outliers=d_outliers)
