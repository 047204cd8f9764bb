"""numpy / scipy statement of the Rician debias (preproc.py:8-36), for the tests.

Per voxel: sigma = mean(S[b0_idx]) / SNR (the mean in the samples' own precision, as numpy takes it), and over E
    F(E) = sum_i (S_i - mu(E_i))^2,   mu(e) = |sigma| sqrt(pi/2) L_{1/2}(-e^2 / (2 sigma^2)).
F is separable, mu is increasing and convex on e >= 0 with mu(0) = |sigma| sqrt(pi/2) (the noise floor), so the
minimiser is mu^{-1}(S_i) above the floor and 0 at or below it.
"""
import numpy as np
from scipy.optimize import brentq
from scipy.special import ive

SQRT_HALF_PI = np.sqrt(np.pi / 2.0)
X_ASYMPTOTIC = 1e4


def sigma_of(S, b0_idx, snr):
    """float64 [n]: b0 mean of every row in the rows' precision (preproc.py:30), divided by the SNR in float64"""
    S = np.asarray(S)
    b0 = np.array([S[i, b0_idx].mean() for i in range(S.shape[0])], dtype=S.dtype)
    return b0.astype(np.float64) / float(snr)


def floor_of(sigma):
    return np.abs(sigma) * SQRT_HALF_PI


def mu(e, sigma):
    """mean of a Rician variable of underlying amplitude e and noise sigma (broadcast), float64"""
    e, s = np.broadcast_arrays(np.asarray(e, dtype=np.float64), np.abs(np.asarray(sigma, dtype=np.float64)))
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        x = e * e / (2.0 * s * s)
        big = x > X_ASYMPTOTIC
        xs = np.where(big, 1.0, x)
        closed = s * SQRT_HALF_PI * ((1.0 + xs) * ive(0, xs / 2.0) + xs * ive(1, xs / 2.0))
        xb = np.where(big, x, 1.0)
        series = np.abs(e) * (1.0 + 1.0 / (4.0 * xb) + 1.0 / (32.0 * xb * xb))
    return np.where(big, series, closed)


def objective(E, S, sigma):
    """F per voxel: E, S [n, nS], sigma [n]"""
    r = np.asarray(S, dtype=np.float64) - mu(E, np.asarray(sigma)[:, None])
    return np.sum(r * r, axis=1)


def exact_minimiser(S, sigma):
    """sample by sample: brentq on mu(e) - S over [0, S] above the floor, 0 at or below it; sigma == 0 rows unchanged"""
    S = np.asarray(S, dtype=np.float64)
    E = np.zeros_like(S)
    fl = floor_of(sigma)
    for i in range(S.shape[0]):
        if not (sigma[i] != 0.0 and np.isfinite(sigma[i])):
            E[i] = S[i]
            continue
        for j in range(S.shape[1]):
            s = S[i, j]
            if s > fl[i]:
                E[i, j] = brentq(lambda e: float(mu(e, sigma[i])) - s, 0.0, s, xtol=1e-300, rtol=8.9e-16, maxiter=500)
    return E


def bisect_minimiser(S, sigma, iters=64):
    """the same minimiser by vectorised bisection of mu(e) - S on [0, S] (64 halvings: to the last bit of S); for many samples"""
    S = np.asarray(S, dtype=np.float64)
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64)[:, None], S.shape)
    above = S > floor_of(sg)
    lo, hi = np.zeros_like(S), np.where(above, S, 0.0)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        up = mu(mid, sg) < S
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return np.where(above, 0.5 * (lo + hi), 0.0)
