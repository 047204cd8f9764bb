"""numpy restatement of the tensor maps dipy's TensorModel gives (test infrastructure only): dipy/reconst/dti.py, dipy >= 1.4.1.

    TensorModel.__init__     min_diffusivity = 1e-6 / -design_matrix.min()
    TensorModel.fit          params of the fit method (tests/dti_methods_np.py: ols_params, wls_params, nlls_params), then
    decompose_tensor         eigh, eigenvalues re-sorted in descending order, clipped from below at min_diffusivity
    fractional_anisotropy    sqrt(1/2 ((e1-e2)^2 + (e2-e3)^2 + (e3-e1)^2) / (e1^2 + e2^2 + e3^2)), 0 where the eigenvalues are all 0
    mean_diffusivity         (e1 + e2 + e3) / 3;  axial_diffusivity e1;  radial_diffusivity (e2 + e3) / 2

dipy is not installed here: tests/test_dti_maps.py pins this file on tensors whose eigenvalues and FA are known in closed form.
"""
import numpy as np

import dti_methods_np as M

MIN_DIFFUSIVITY_TOL = 1e-6
SMALL_SHARE = 1e-3          # scalars are held to their bounds where the largest clipped eigenvalue is >= this share of max |D entry|


def min_diffusivity(X):
    return MIN_DIFFUSIVITY_TOL / -X.min()


def params(y, X, method, min_signal=None, tight=False):
    if method in ('OLS', 'LS'):
        return M.ols_params(y, X, min_signal)
    if method == 'WLS':
        return M.wls_params(y, X, min_signal)
    if method == 'NLLS':
        return M.nlls_params(y, X, min_signal, tight=tight)
    raise ValueError(method)


def scalars(evals):
    """clipped eigenvalues [n, 3], descending -> [n, 4] = FA, MD, AD, RD"""
    e1, e2, e3 = evals[:, 0], evals[:, 1], evals[:, 2]
    all_zero = (evals == 0).all(axis=1)
    with np.errstate(invalid='ignore'):
        fa = np.sqrt(0.5 * ((e1 - e2) ** 2 + (e2 - e3) ** 2 + (e3 - e1) ** 2) / ((evals * evals).sum(axis=1) + all_zero))
    return np.stack([fa, (e1 + e2 + e3) / 3.0, e1, 0.5 * (e2 + e3)], axis=1)


def maps_of_params(p, min_diff):
    """[n, 7] parameters -> dict(directions, evals (clipped), scalars, scale = largest |tensor entry| of each voxel)"""
    dirs, ev = M.decompose(p)
    ev = np.where(ev < min_diff, min_diff, ev)            # decompose_tensor: evals.clip(min=min_diffusivity)
    return {'directions': dirs, 'evals': ev, 'scalars': scalars(ev), 'scale': np.abs(p[:, :6]).max(axis=1), 'params': p}


def fit_maps(y, bvals, bvecs, method='OLS', min_signal=None, tight=False):
    """TensorModel(gtab, fit_method=method).fit(y): .directions, .evals, (.fa, .md, .ad, .rd)"""
    X = M.design(bvals, bvecs)
    return maps_of_params(params(y, X, method, min_signal, tight), min_diffusivity(X))


def held(ref):
    """voxels whose scalars are held to the bounds: the clip has not taken over (largest clipped eigenvalue >= 1e-3 of the tensor's scale)"""
    return ref['evals'][:, 0] >= SMALL_SHARE * ref['scale']


def table(scheme, merge_b0=False):
    """(bvals, bvecs) of the tensor fit: the scheme's, or with doMergeB0 [one b0] + the DWI volumes (core.py:428-432)"""
    b, g = np.asarray(scheme.b, dtype=float), np.asarray(scheme.raw, dtype=float)[:, :3]
    if merge_b0:
        b, g = np.hstack((0.0, b[scheme.dwi_idx])), np.vstack((np.zeros((1, 3)), g[scheme.dwi_idx]))
    return b, g


def merge_b0(y, scheme):
    return np.hstack([y[:, scheme.b0_idx].mean(axis=1, keepdims=True), y[:, scheme.dwi_idx]])


# ----------------------------------------------------------------------------- the scenes the CPU and the GPU tests share
N_VOX = 1029                # one voxel more than 16 tiles of 64 (and 25 tiles of 40 + 29 on the 200-volume scheme)


def _six_direction_scheme():
    """the shortest scheme the fit accepts, 7 volumes: one b0 and the six icosahedral directions (the classic minimal DTI protocol)"""
    from amico_amd.synthetic import SimpleScheme
    phi = (1.0 + np.sqrt(5.0)) / 2.0
    g = np.array([[0, 1, phi], [0, 1, -phi], [1, phi, 0], [-1, phi, 0], [phi, 0, 1], [phi, 0, -1]]) / np.sqrt(1.0 + phi * phi)
    return SimpleScheme(np.vstack([np.zeros(4), np.hstack([g, np.full((6, 1), 1000.0)])]))


def scene(name):
    """name -> (scheme, doMergeB0): 'std' the 99-volume make_scheme(), 'merge' the same with doMergeB0 (91 volumes), 'short' 7 volumes,
    'long' 200 volumes (tiles of 40 voxels instead of 64)"""
    import amico_amd.synthetic as S
    if name in ('std', 'merge'):
        return S.make_scheme(), name == 'merge'
    if name == 'short':
        return _six_direction_scheme(), False
    if name == 'long':
        return S.make_scheme(n_b0=10, shells=((1000.0, 60), (2000.0, 70), (3000.0, 60)), seed=5), False
    raise KeyError(name)


SCENES = ('std', 'merge', 'short', 'long')
_cache = {}


def scene_signals(name, htable500):
    """(bvals, bvecs, y f64 [N_VOX, nS]) of a scene: synthetic NODDI signals (Rician noise, SNR 30) rounded to float32, so that the
    float32 and the float64 rows of a test hold the same numbers and share one reference.  Computed once, never modified."""
    import amico_amd.synthetic as S
    if ('y', name) not in _cache:
        sc, merge = scene(name)
        K = S.noddi_kernels(sc, htable500['dirs'])
        y, _ = S.noddi_signals(N_VOX, K, htable500['htable'], sc, seed=21)
        if merge:
            y = merge_b0(y, sc)
        y = np.ascontiguousarray(y.astype(np.float32).astype(np.float64))
        y.setflags(write=False)
        _cache['y', name] = table(sc, merge) + (y,)
    return _cache['y', name]


def scene_reference(name, method, htable500):
    """the restatement on a scene's signals; for NLLS MINPACK run to 1e-15 ('tight') with the eigenvalues MINPACK leaves at dipy's
    default tolerances beside it ('evals_default', 'scalars_default')"""
    if ('ref', name, method) not in _cache:
        b, g, y = scene_signals(name, htable500)
        ref = fit_maps(y, b, g, method, tight=True)
        if method == 'NLLS':
            dflt = fit_maps(y, b, g, method)
            ref['evals_default'], ref['scalars_default'] = dflt['evals'], dflt['scalars']
        for a in ref.values():
            a.setflags(write=False)
        _cache['ref', name, method] = ref
    return _cache['ref', name, method]
