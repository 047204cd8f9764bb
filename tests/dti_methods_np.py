"""numpy restatement of dipy's weighted and non-linear tensor fits (test infrastructure only).

dipy is not installed here, so what follows restates its published routines with the numpy / scipy calls they make
(dipy/reconst/dti.py, dipy >= 1.4.1): `wls_fit_tensor` and `nlls_fit_tensor` (weighting=None), followed by
`decompose_tensor`.  X = design_matrix(gtab), s = max(y, min_signal).

  WLS   p_ols = pinv(X) log s;  w = exp(X p_ols);  p = pinv(X * w[:, None]) @ (w * log s)
  NLLS  MINPACK's Levenberg-Marquardt (scipy.optimize.leastsq) on r(p) = s - exp(X p) with the analytic Jacobian
        -exp(X p)[:, None] * X, started from the OLS parameters; a failed solve keeps the starting parameters.
        dipy passes MINPACK's default tolerances (`nlls(y, X)`); `tight=True` runs the same call down to
        ftol = xtol = 1e-15, i.e. to the minimum itself.

The fixture tests/golden/dti_methods_fixture.npz pins both against routes that share no code with this file.
"""
import numpy as np

from oracle.signal_np import MIN_POSITIVE_SIGNAL, design_matrix, gradient_table

_LT = np.array([[0, 1, 3], [1, 2, 4], [3, 4, 5]])                        # from_lower_triangular


def _data(y, X, min_signal):
    return np.maximum(np.asarray(y, dtype=float).reshape(-1, X.shape[0]), MIN_POSITIVE_SIGNAL if min_signal is None else min_signal)


def ols_params(y, X, min_signal=None):
    return np.log(_data(y, X, min_signal)) @ np.linalg.pinv(X).T


def wls_params(y, X, min_signal=None):
    data = _data(y, X, min_signal)
    log_s = np.log(data)
    w = np.exp(log_s @ (X @ np.linalg.pinv(X)).T)                        # exp(X p_ols)
    p = np.empty((len(data), 7))
    for i in range(len(data)):
        p[i] = np.linalg.pinv(X * w[i][:, None]) @ (w[i] * log_s[i])
    return p


def nlls_params(y, X, min_signal=None, tight=False):
    import scipy.optimize as opt
    data = _data(y, X, min_signal)
    start = ols_params(y, X, min_signal)

    def err(p, s):
        return s - np.exp(X @ p)

    def jac(p, s):
        return -np.exp(X @ p)[:, None] * X

    kw = dict(ftol=1e-15, xtol=1e-15, gtol=0.0, maxfev=4000) if tight else {}
    p = np.empty_like(start)
    for i in range(len(data)):
        try:
            with np.errstate(all='ignore'):
                p[i] = opt.leastsq(err, start[i], args=(data[i],), Dfun=jac, **kw)[0]
            if not np.all(np.isfinite(p[i])):
                p[i] = start[i]
        except (np.linalg.LinAlgError, ValueError):
            p[i] = start[i]
    return p


def decompose(p):
    """decompose_tensor: eigh, re-sorted in descending order -> (principal axes [n, 3], evals [n, 3])"""
    evals, evecs = np.linalg.eigh(p[:, _LT])
    order = np.argsort(evals, axis=1)[:, ::-1]
    first = order[:, 0]
    return evecs[np.arange(len(first)), :, first], np.take_along_axis(evals, order, axis=1)


def design(bvals, bvecs):
    return design_matrix(*gradient_table(bvals, bvecs))


def directions(y, bvals, bvecs, method, min_signal=None, tight=False, return_evals=False):
    """np.squeeze(TensorModel(gtab, fit_method=method).fit(y).directions) for method in 'OLS' | 'WLS' | 'NLLS'"""
    X = design(bvals, bvecs)
    if method in ('OLS', 'LS'):
        p = ols_params(y, X, min_signal)
    elif method == 'WLS':
        p = wls_params(y, X, min_signal)
    elif method == 'NLLS':
        p = nlls_params(y, X, min_signal, tight=tight)
    else:
        raise ValueError(method)
    dirs, evals = decompose(p)
    return (dirs, evals) if return_evals else dirs
