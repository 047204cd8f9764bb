"""numpy restatement of the noise estimate from the b0 repeats (include/amico_amd.h, "(f0+)"): what the kernels are held to,
bit for bit.  Sums run sequentially over the k columns with an explicit loop (np.sum pairs its terms differently); every numpy
operation on float64 arrays is rounded on its own, like the kernel's."""
import numpy as np
from scipy import special


def per_voxel(S, b0_idx):
    """S [n, nS] float32 | float64 -> (mean, sd, ratio) float64 [n], NaN in all three where the voxel is not eligible"""
    S = np.asarray(S)
    b0_idx = [int(i) for i in b0_idx]
    k = len(b0_idx)
    x = [S[:, i].astype(np.float64) for i in b0_idx]
    with np.errstate(all='ignore'):
        total = x[0].copy()
        finite = np.isfinite(x[0])
        for i in range(1, k):
            total = total + x[i]
            finite &= np.isfinite(x[i])
        m = total / np.float64(k)
        q = (x[0] - m) * (x[0] - m)
        for i in range(1, k):
            d = x[i] - m
            q = q + d * d
        sd = np.sqrt(q / np.float64(k - 1))
        ok = finite & (m > 0) & (sd > 0) & np.isfinite(sd)
        ratio = m / sd
    nan = np.float64('nan')
    return np.where(ok, m, nan), np.where(ok, sd, nan), np.where(ok, ratio, nan)


def chi2_median_ratio(nu):
    return float(2.0 * special.gammaincinv(0.5 * nu, 0.5) / nu)


def estimate(S, b0_idx):
    """-> {'snr', 'sigma', 'voxels', 'mean', 'sd'} as amico_amd.noise.estimate_from_rows returns them"""
    mean, sd, ratio = per_voxel(S, b0_idx)
    c = int((~np.isnan(sd)).sum())
    if c == 0:
        return {'snr': float('nan'), 'sigma': float('nan'), 'voxels': 0, 'mean': mean, 'sd': sd}
    root = np.sqrt(chi2_median_ratio(len(b0_idx) - 1))
    return {'snr': float(np.nanmedian(ratio) * root), 'sigma': float(np.nanmedian(sd) / root), 'voxels': c, 'mean': mean, 'sd': sd}


def key(v):
    """the order-preserving uint64 key of float64 values: sign bit set -> all bits flipped; otherwise the sign bit flipped"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b ^ np.uint64(1 << 63))


def middles(v):
    """-> (lower middle, upper middle, count) of the non-NaN values of v, by np.partition on the keys (so that -0.0 sorts before +0.0
    and equal values keep their bit patterns); NaN, NaN, 0 when there is none"""
    v = np.asarray(v, dtype=np.float64).ravel()
    kk = key(v[~np.isnan(v)])
    c = kk.size
    if c == 0:
        return np.float64('nan'), np.float64('nan'), 0
    lo, hi = (c - 1) // 2, c // 2
    part = np.partition(kk, (lo, hi))

    def value(u):
        u = np.uint64(u)
        b = (u ^ np.uint64(1 << 63)) if (u >> np.uint64(63)) else ~u
        return np.array([b], dtype=np.uint64).view(np.float64)[0]
    return value(part[lo]), value(part[hi]), c
