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


LD = np.longdouble


def _dual(res, A):
    """res' A in float64 from a long-double residual res [n, rows]: its float64 head and tail multiplied apart (the products' own
    rounding is eps |res| |A| rows, ten thousand times below any bound used with it)"""
    hi = res.astype(np.float64)
    lo = (res - hi).astype(np.float64)
    return hi @ A + lo @ A


def noddi_certificates_per_voxel(K, sch, ht, y, d, x, lam1, lam2, exvivo=False):
    """noddi_certificates voxel by voxel and relative to s = max|y| of the voxel, every residual formed in long double: a dict of [n]
    arrays -- 's', per stage k = 1, 2, 3 'min_x<k>', 'gP<k>' (max |dual| on the passive atoms / s) and 'gZ<k>' (largest positive dual
    on the clamped atoms / s; stage 3: of the allowed set), 'off3' (largest |stage-3 coefficient| outside the allowed set: the stage-2
    support of x ITSELF + the dot atom + iso) -- and 'g2' [n, n_wm], the stage-2 dual vector as it is.  All-zero voxels (s = 0) report
    the absolute values.  The stage-2 signal is made of the stage-1 coefficients of x itself (models.pyx:914-926)."""
    from amico_amd import synthetic as S
    lut = S.lut_indices(d, ht)
    n, n_wm = len(y), K['wm'].shape[0]
    iso = K['iso'].astype(np.float64)
    fixed = ([np.ones_like(iso)] if exvivo else []) + [iso]
    dwi = np.asarray(sch.dwi_idx)
    norms = K['norms'][0]
    s = np.abs(y).max(axis=1)
    sc = np.where(s > 0, s, 1.0)
    out = {k: np.zeros(n) for k in ('min_x1', 'gP1', 'gZ1', 'min_x2', 'gP2', 'gZ2', 'min_x3', 'gP3', 'gZ3', 'off3')}
    out['s'] = s
    out['g2'] = np.zeros((n, n_wm))

    def put(stage, rows, X, G, P, Z):
        out['min_x%d' % stage][rows] = X.min(axis=1)
        out['gP%d' % stage][rows] = np.where(P, np.abs(G), 0.0).max(axis=1) / sc[rows]
        out['gZ%d' % stage][rows] = np.maximum(np.where(Z, G, 0.0).max(axis=1), 0.0) / sc[rows]
    for rows in by_direction(lut):
        A = np.concatenate([K['wm'][:, lut[rows[0]], :].astype(np.float64)] + [f[None, :] for f in fixed], axis=0).T      # nS x n_atoms
        Al = A.astype(LD)
        Y = y[rows].astype(LD)
        x1, x2, x3 = x[rows, 0], x[rows, 1, :n_wm], x[rows, 2]
        W = _dual(Y - x1.astype(LD) @ Al.T, A)
        put(1, rows, x1, W, x1 > 0, x1 <= 0)
        A2 = A[dwi][:, :n_wm] * norms[None, :]
        Y2 = np.maximum(Y[:, dwi] - x1[:, n_wm:].astype(LD) @ Al[dwi][:, n_wm:].T, LD(0))
        G = _dual(Y2 - x2.astype(LD) @ A2.astype(LD).T, A2) - lam2 * x2 - lam1
        P = x2 > 0
        put(2, rows, x2, G, P, ~P)
        out['g2'][rows] = G
        allowed = np.concatenate([P, np.ones((len(rows), len(fixed)), dtype=bool)], axis=1)
        W = _dual(Y - x3.astype(LD) @ Al.T, A)
        put(3, rows, x3, W, x3 > 0, allowed & (x3 <= 0))
        out['off3'][rows] = np.where(allowed, 0.0, np.abs(x3)).max(axis=1)
    return out
