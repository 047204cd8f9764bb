"""numpy restatement of the predicted signal y_est = A x (include/amico_amd.h: amx_predict_device), the reference of tests/test_predicted.py
and tests/test_gpu_predicted.py: fp64, atoms in ascending order, one rounding per product and per sum -- numpy's elementwise `*` and
`+` are exactly that.  A_i and x_i are what the reference hands to _compute_rmse for voxel i (models.pyx:47-71)."""
import numpy as np


def columns(K):
    """the atoms of KERNELS in the dictionary's column order: a list of [ndirs, nS] (rotated) or [nS] (isotropic) arrays"""
    model = K['model']
    if model == 'NODDI':                                   # [wm | iso]                       models.pyx:905-908
        return list(K['wm']) + [K['iso']]
    if model == 'FreeWater':                               # [D | CSF]                        models.pyx:1230-1233
        return list(K['D']) + list(K['CSF'])
    if model == 'SANDI':                                   # KERNELS['signal']                models.pyx:1569
        return list(np.asarray(K['signal']).T)
    if model == 'CylinderZeppelinBall':                    # [wmr | wmh | iso]                models.pyx:608-610
        return list(K['wmr']) + list(K['wmh']) + list(K['iso'])
    raise ValueError(model)


def lut_index(dirs, htable, ndirs):
    """orientation of every voxel (lut.pyx:316-356, the oracle's), -1 where the fit skips the voxel"""
    from oracle import oracle
    idx = oracle.dir_to_lut_idx(dirs, htable)[0].astype(np.int64)
    idx[(idx < 0) | (idx >= ndirs)] = -1
    return idx


def predict_rows(K, x, idx=None):
    """x f64 [n, n_atoms], idx int [n] (None: a model without orientations) -> y_est f64 [n, nS]:
    acc = 0; for j: acc = acc + A[..., j] * x[:, j:j+1]; a voxel with idx < 0 gets zeros"""
    cols = columns(K)
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[1] == len(cols)
    safe = None if idx is None else np.where(idx < 0, 0, idx)
    acc = np.zeros((x.shape[0], cols[0].shape[-1]))
    with np.errstate(invalid='ignore'):
        for j, c in enumerate(cols):
            a = np.asarray(c, dtype=np.float64)
            a = a[safe] if a.ndim == 2 else a[None, :]
            acc = acc + a * x[:, j:j + 1]
    if idx is not None:
        acc[idx < 0] = 0.0
    return acc


def dense_dictionaries(K, idx=None, n=None):
    """A f64 [n, nS, n_atoms] of every voxel, for small cases (A @ x)"""
    cols = columns(K)
    per = []
    for c in cols:
        a = np.asarray(c, dtype=np.float64)
        per.append(a[idx] if a.ndim == 2 else np.broadcast_to(a, (len(idx) if idx is not None else n,) + a.shape))
    return np.stack(per, axis=2)
