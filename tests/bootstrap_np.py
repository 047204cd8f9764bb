"""numpy restatement of the wild bootstrap's three kernels (include/amico_amd.h: amx_bootstrap_*): the sign generator, the replicate
signal and Welford's moments, operation by operation in the order the header states -- what the GPU results are held to bit for bit."""
import numpy as np

U = np.uint64
GOLDEN, WEYL = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03


def signs(seed, b, first_voxel, n, nS):
    """+-1.0 [n, nS]: the Rademacher weights of replicate b for voxels first_voxel .. first_voxel + n - 1"""
    with np.errstate(over='ignore'):
        ctr = (np.arange(n, dtype=U)[:, None] + U(first_voxel)) * U(nS) + np.arange(nS, dtype=U)[None, :]
        z = U(seed) + U(b + 1) * U(GOLDEN) + ctr * U(WEYL)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        z = z ^ (z >> U(31))
    return np.where((z >> U(63)) != 0, -1.0, 1.0)


def resample(y, y_est, seed, b, first_voxel=0):
    """the replicate signal in the dtype of y (float32 | float64): max(0, y_est + s (y - y_est)) in fp64, a NaN stays"""
    y = np.asarray(y)
    assert y.dtype in (np.float32, np.float64) and y_est.dtype == np.float64 and y.shape == y_est.shape
    s = signs(seed, b, first_voxel, *y.shape)
    with np.errstate(invalid='ignore'):
        v = y_est + s * (y.astype(np.float64) - y_est)
        v = np.where(v < 0, 0.0, v)
    return v.astype(y.dtype)


def welford(maps):
    """(mean, std) over a list of B >= 2 equally shaped float64 arrays: d = m - mean; mean += d / t; M2 += d (m - mean);
    std = sqrt(M2 / (B - 1))"""
    mean = np.zeros_like(maps[0], dtype=np.float64)
    m2 = np.zeros_like(mean)
    with np.errstate(invalid='ignore'):
        for t, m in enumerate(maps, 1):
            d = m - mean
            mean = mean + d / np.float64(t)
            m2 = m2 + d * (m - mean)
        return mean, np.sqrt(m2 / np.float64(len(maps) - 1))
