"""Kuhn-Tucker certificates of the NODDI fit computed in numpy from the device coefficient vectors (AMX_F_DEBUG_X) alone:
shared by the GPU test modules (test_gpu_kkt.py, test_gpu_amplitude.py)."""
import numpy as np


def by_direction(lut_idx):
    order = np.argsort(lut_idx, kind='stable')
    bounds = np.flatnonzero(np.diff(lut_idx[order])) + 1
    return np.split(order, bounds)


def noddi_certificates(K, sch, ht, y, d, x, lam1, lam2, exvivo=False):
    """max KKT violations of the three NODDI solves, from the device coefficients only (exvivo: the dot atom -- a column of
    ones, models.pyx:843-844 -- sits between the wm atoms and iso)"""
    from amico_amd import synthetic as S
    lut = S.lut_indices(d, ht)
    n_wm = K['wm'].shape[0]
    iso = K['iso'].astype(np.float64)
    fixed = ([np.ones_like(iso)] if exvivo else []) + [iso]
    dwi = np.asarray(sch.dwi_idx)
    norms = K['norms'][0]
    out = {k: 0.0 for k in ('s1_wP', 's1_wZ', 's2_gP', 's2_gZ', 's3_wP', 's3_wZ', 's3_off_support')}
    neg = 0.0
    for rows in by_direction(lut):
        A = np.concatenate([K['wm'][:, lut[rows[0]], :].astype(np.float64)] + [f[None, :] for f in fixed], axis=0).T      # nS x n_atoms
        Y = y[rows]
        x1, x2, x3 = x[rows, 0], x[rows, 1], x[rows, 2]
        neg = min(neg, x1.min(), x2.min(), x3.min())
        # stage 1: NNLS over all atoms
        W = (Y - x1 @ A.T) @ A
        P = x1 > 0
        out['s1_wP'] = max(out['s1_wP'], np.abs(W[P]).max(initial=0.0))
        out['s1_wZ'] = max(out['s1_wZ'], W[~P].max(initial=0.0))
        # stage 2: non-negative elastic net on the column-normalised wm atoms, y2 clipped (models.pyx:914-926)
        A2 = A[dwi][:, :n_wm] * norms[None, :]
        Y2 = np.maximum(Y[:, dwi] - x1[:, n_wm:] @ A[dwi][:, n_wm:].T, 0.0)
        xl = x2[:, :n_wm]
        G = (Y2 - xl @ A2.T) @ A2 - lam2 * xl - lam1
        P = xl > 0
        out['s2_gP'] = max(out['s2_gP'], np.abs(G[P]).max(initial=0.0))
        out['s2_gZ'] = max(out['s2_gZ'], G[~P].max(initial=0.0))
        # stage 3: NNLS on the LASSO support + iso (models.pyx:929-942)
        allowed = np.concatenate([P, np.ones((len(rows), len(fixed)), dtype=bool)], axis=1)
        W = (Y - x3 @ A.T) @ A
        P3 = x3 > 0
        out['s3_off_support'] = max(out['s3_off_support'], np.abs(x3[~allowed]).max(initial=0.0))
        out['s3_wP'] = max(out['s3_wP'], np.abs(W[P3]).max(initial=0.0))
        out['s3_wZ'] = max(out['s3_wZ'], W[allowed & ~P3].max(initial=0.0))
    out['min_x'] = float(neg)
    return out
