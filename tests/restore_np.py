"""numpy / scipy restatement of the robust tensor fit, DTI_fit_method 'RT' | 'RESTORE' | 'restore' with a noise level sigma (test
infrastructure only; include/amico_amd.h states the algorithm, steps 1-5).

`restore` is the project's algorithm.  X = design_matrix(gtab), s = max(y, min_signal):

  1. p1 = NLLS (dti_methods_np.nlls_params run tight: MINPACK to ftol = xtol = 1e-15)
  2. r = s - exp(X p1); no |r_i| > 3 sigma: done
  3. the Geman-McClure fit as a fixed point from p1.  `route='trial'`: per trip the weights are taken at p and ONE
     Levenberg-Marquardt trial is made on the frozen-weight cost (what the kernel does).  `route='converged'`: per trip the frozen-weight
     problem is solved to its minimum by MINPACK before the weights move (Chang, Jones & Pierpaoli 2005 as usually written).
  4. r = s - exp(X p2), O = {|r_i| > 3 sigma}; empty: p2; fewer than 7 samples left: p2; else WLS start and tight NLLS on the rest
  5. tensor -> axis, eigenvalues

`restore_dipy_route` restates what dipy's restore_fit_tensor itself does in step 3 -- MINPACK on a cost whose Geman-McClure weights are
recomputed at every evaluation, with the Jacobian of the unweighted residuals -- for the record only: it has no defined fixed point
that a second implementation could be held to, which is why the project does not follow it.
"""
import numpy as np

import dti_methods_np as M

TRIP_CAP = 1024
_TIGHT = dict(ftol=1e-15, xtol=1e-15, gtol=0.0, maxfev=4000)


def gm_weights(r, sigma):
    """Geman-McClure weights of the residuals r, normalised to mean 1"""
    C = max(1.4826 * np.median(np.abs(r - np.median(r))), 1e-6 * sigma)
    w = 1.0 / (r * r + C * C)
    return w / w.mean()


def _trial_route(s, X, p, sigma, cap):
    """-> (p2, trips, capped): one Levenberg-Marquardt trial per trip on sum w_i (s_i - exp(X_i p))^2, w frozen at p"""
    lam = 1e-3
    for trip in range(1, cap + 1):
        e = np.exp(X @ p)
        r = s - e
        w = gm_weights(r, sigma)
        J = e[:, None] * X
        G = J.T @ (w[:, None] * J)
        g = J.T @ (w * r)
        c = np.sum(w * r * r)
        try:
            d = np.linalg.solve(G + lam * np.diag(np.diag(G)), g)
            rt = s - np.exp(X @ (p + d))
            ct = np.sum(w * rt * rt)
            ok = np.all(np.isfinite(d)) and ct <= c
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            p = p + d
            lam = max(lam * 0.1, 1e-12)
            if np.abs(X @ d).max() <= 1e-10:
                return p, trip, False
        else:
            lam *= 10.0
            if lam > 1e12:
                return p, trip, True
    return p, cap, True


def _converged_route(s, X, p, sigma, cap=200):
    """-> (p2, trips, capped): every frozen-weight problem solved by MINPACK before the weights move"""
    import scipy.optimize as opt
    for trip in range(1, cap + 1):
        sw = np.sqrt(gm_weights(s - np.exp(X @ p), sigma))
        new = opt.leastsq(lambda q: sw * (s - np.exp(X @ q)), p, Dfun=lambda q: -(sw * np.exp(X @ q))[:, None] * X, **_TIGHT)[0]
        moved = np.abs(X @ (new - p)).max()
        p = new
        if moved <= 1e-10:
            return p, trip, False
    return p, cap, True


def restore(y, X, sigma, min_signal=None, route='trial', cap=TRIP_CAP):
    """-> dict: 'params' [n, 7], 'outliers' int [n], 'mask' bool [n, nS] (the samples left out), 'entered' / 'refitted' / 'capped' /
    'few' bool [n], 'trips' int [n], 'margin' [n]: min_i | |r_i| - 3 sigma | / sigma over the verdicts the voxel went through (how far
    the nearest sample was from changing sides)"""
    import scipy.optimize as opt
    s_all = M._data(y, X, min_signal)
    n, nS = s_all.shape
    p1 = M.nlls_params(y, X, min_signal, tight=True)
    out = dict(params=p1.copy(), outliers=np.zeros(n, dtype=int), mask=np.zeros((n, nS), dtype=bool), trips=np.zeros(n, dtype=int),
               margin=np.full(n, np.inf))
    for key in ('entered', 'refitted', 'capped', 'few'):
        out[key] = np.zeros(n, dtype=bool)
    thr = 3.0 * sigma
    for i in range(n):
        s = s_all[i]
        with np.errstate(all='ignore'):
            r = s - np.exp(X @ p1[i])
        if not np.all(np.isfinite(r)):
            continue
        out['margin'][i] = np.abs(np.abs(r) - thr).min() / sigma
        if not np.any(np.abs(r) > thr):
            continue
        out['entered'][i] = True
        with np.errstate(all='ignore'):
            p2, out['trips'][i], out['capped'][i] = (_trial_route if route == 'trial' else _converged_route)(s, X, p1[i].copy(), sigma, cap)
        out['params'][i] = p2
        r = s - np.exp(X @ p2)
        out['margin'][i] = min(out['margin'][i], np.abs(np.abs(r) - thr).min() / sigma)
        O = np.abs(r) > thr
        out['mask'][i], out['outliers'][i] = O, O.sum()
        if not O.any():
            continue
        if nS - O.sum() < 7:
            out['few'][i] = True
            continue
        out['refitted'][i] = True
        Xc, sc = X[~O], s[~O]
        start = M.wls_params(sc[None, :], Xc, min_signal)[0]
        with np.errstate(all='ignore'):
            p = opt.leastsq(lambda q: sc - np.exp(Xc @ q), start, Dfun=lambda q: -np.exp(Xc @ q)[:, None] * Xc, **_TIGHT)[0]
        out['params'][i] = p if np.all(np.isfinite(p)) else start
    return out


def refit_default(y, X, mask, min_signal=None):
    """MINPACK at dipy's default tolerances from the OLS start on each voxel's samples outside `mask`: the yardstick of
    test_dti_methods._nlls_check, on the inlier sets of a robust fit"""
    s_all = M._data(y, X, min_signal)
    p = np.empty((len(s_all), 7))
    for i, s in enumerate(s_all):
        keep = ~mask[i]
        p[i] = M.nlls_params(s[keep][None, :], X[keep], min_signal)[0]
    return p


def restore_dipy_route(y, X, sigma, min_signal=None):
    """dipy's own route (restore_fit_tensor): -> (params [n, 7], mask bool [n, nS])"""
    import scipy.optimize as opt
    s_all = M._data(y, X, min_signal)
    start_all = M.ols_params(y, X, min_signal)
    params, mask = start_all.copy(), np.zeros(s_all.shape, dtype=bool)

    def jac(q, Xq, sq, weighting):
        return -np.exp(Xq @ q)[:, None] * Xq

    def err(q, Xq, sq, weighting):
        r = sq - np.exp(Xq @ q)
        if weighting == 'sigma':
            return r / sigma
        C = 1.4826 * np.median(np.abs(r - np.median(r)))
        with np.errstate(all='ignore'):
            w = 1.0 / (r * r + C * C)
            return np.sqrt(w / w.mean() * r * r)

    for i, s in enumerate(s_all):
        p = opt.leastsq(err, start_all[i], args=(X, s, 'sigma'), Dfun=jac)[0]
        if np.any(np.abs(s - np.exp(X @ p)) > 3.0 * sigma):
            p = opt.leastsq(err, start_all[i], args=(X, s, 'gmm'), Dfun=jac)[0]
            O = np.abs(s - np.exp(X @ p)) > 3.0 * sigma
            mask[i] = O
            if O.any() and (~O).sum() >= 7:
                Xc, sc = X[~O], s[~O]
                p = opt.leastsq(err, M.wls_params(sc[None, :], Xc, min_signal)[0], args=(Xc, sc, 'sigma'), Dfun=jac)[0]
        params[i] = p
    return params, mask
