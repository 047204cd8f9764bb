"""numpy side of the Marchenko-Pastur denoiser (include/amico_amd.h, "(f0+++)"), shared by tests/test_mppca_denoise.py and
tests/test_gpu_mppca_denoise.py:
  reference   per voxel the float64 numpy.linalg.svd of its patch matrix X truncated at rank s, column c; s from mppca_np.rule on
              numpy.linalg.eigvalsh of the Gram matrix
  restated    the kernel's own algorithm: reflectors kept, b' = Q^T b, twisted-factorisation eigenvectors of the smaller set from the
              bisected eigenvalues, Gram-Schmidt twice, projection or complement, z = Q z', x^ = z | X z
  highrank    images that mix K profiles at random per voxel (mppca_np.synthetic has rank <= 6 whatever `components` says)"""
import numpy as np

import mppca_np as M

EPS = 2.0 ** -52


def centre_column(sel, centre, w):
    """index of the voxel itself among its cube's masked columns (C order of the cube)"""
    s = [M.cube_start(int(centre[a]), sel.shape[a], w) for a in range(3)]
    cube = sel[s[0]:s[0] + w, s[1]:s[1] + w, s[2]:s[2] + w]
    pos = np.ravel_multi_index(tuple(int(centre[a]) - s[a] for a in range(3)), (w, w, w))
    return int(cube.ravel()[:pos].sum())


def truncated_column(X, s, col):
    """column col of the best approximation of rank s of X, by the float64 SVD"""
    U, sv, Vt = np.linalg.svd(X, full_matrices=False)
    return (U[:, :s] * sv[:s]) @ Vt[:s, col]


def reference(img, mask, w):
    """-> dict over the voxels of mask == 1 in C order: 'status' int32 (0 denoised, 1 not eligible), 'rows' f64 [n_vox, nS] (NaN where
    status != 0), 'signal', 'r', 'q', 'lam_max', 'gap' (lambda[cut] - lambda[cut - 1]; inf when s = 0), 'norm' (|x_c|), 'margin'"""
    img = np.asarray(img)
    sel = np.asarray(mask) == 1
    cs = np.argwhere(sel)
    nv, nS = len(cs), img.shape[3]
    out = {k: np.full(nv, np.nan) for k in ('signal', 'r', 'q', 'lam_max', 'gap', 'norm', 'margin')}
    out['status'] = np.ones(nv, dtype=np.int32)
    out['rows'] = np.full((nv, nS), np.nan)
    for v, c in enumerate(cs):
        X = M.patch_matrix(img, sel, c, w)
        m, n = X.shape
        out['r'][v], out['q'][v] = min(m, n), max(m, n)
        if 2 * n < w ** 3 or not np.all(np.isfinite(X)):
            continue
        G, r, q = M.gram(X)
        lam = np.sort(np.linalg.eigvalsh(G))
        _, nsig, margin, pc = M.rule(lam, q)
        if pc < 0:
            continue
        s, cut = int(nsig), r - int(nsig)
        col = centre_column(sel, c, w)
        out['rows'][v] = truncated_column(X, s, col)
        out['status'][v] = 0
        out['signal'][v], out['lam_max'][v], out['margin'][v] = nsig, lam[-1], margin
        out['gap'][v] = lam[cut] - lam[cut - 1] if s > 0 else np.inf
        out['norm'][v] = np.linalg.norm(X[:, col])
    return out


def bound(ref, c_den):
    """C_DEN eps (q + r) (lambda_max / gap) |x_c| per voxel (NaN where the voxel is not eligible)"""
    return c_den * EPS * (ref['q'] + ref['r']) * (ref['lam_max'] / ref['gap']) * ref['norm']


# ------------------------------------------------------------------ the kernel's algorithm
def tridiagonalise_keep(G):
    """mppca_np.tridiagonalise, keeping the reflectors: -> d, e, V (row k: v of step k over the elements k+1 ..), tau2 [r]"""
    A = np.array(G, dtype=np.float64)
    r = A.shape[0]
    d, e, tau = np.zeros(r), np.zeros(max(r - 1, 0)), np.zeros(r)
    V = np.zeros((r, r))
    for k in range(r - 2):
        b = k + 1
        x = A[k, b:].copy()
        sigma2 = float(x @ x)
        d[k] = A[k, k]
        if not sigma2 > 0.0:
            continue
        norm = np.sqrt(sigma2)
        alpha = -norm if x[0] >= 0.0 else norm
        e[k] = alpha
        tau2 = 1.0 / (sigma2 - alpha * x[0])
        v = x
        v[0] = x[0] - alpha
        V[k, b:], tau[k] = v, tau2
        p = tau2 * (A[b:, b:] @ v)
        w_ = p - 0.5 * tau2 * float(v @ p) * v
        A[b:, b:] -= np.outer(v, w_) + np.outer(w_, v)
    if r >= 2:
        d[r - 2] = A[r - 2, r - 2]
        e[r - 2] = A[r - 1, r - 2]
    d[r - 1] = A[r - 1, r - 1]
    return d, e, V, tau


def twisted_vectors(d, e, lams):
    """eigenvectors of the tridiagonal (d, e) for the eigenvalues lams, one column each, not normalised: forward pivots, backward pivots,
    the twist at the smallest |gamma|, z from the two recurrences; pivots kept 2^-104 of the Gershgorin bound away from zero"""
    r, k = len(d), len(lams)
    ae = np.abs(e)
    rad = np.zeros(r)
    rad[:-1] += ae
    rad[1:] += ae
    pivmin = max(abs(float(np.min(d - rad))), abs(float(np.max(d + rad)))) * 2.0 ** -104
    guard = lambda x: np.where(np.abs(x) < pivmin, -pivmin, x)
    lams = np.asarray(lams, dtype=np.float64)
    dp, dm = np.zeros((r, k)), np.zeros((r, k))
    with np.errstate(all='ignore'):
        dp[0] = guard(d[0] - lams)
        for i in range(1, r):
            dp[i] = guard(d[i] - lams - e[i - 1] * e[i - 1] / dp[i - 1])
        dm[r - 1] = guard(d[r - 1] - lams)
        for i in range(r - 2, -1, -1):
            dm[i] = guard(d[i] - lams - e[i] * e[i] / dm[i + 1])
        gam = np.abs(dp + dm - (d[:, None] - lams[None, :]))
        tw = (r - 1) - np.argmin(gam[::-1], axis=0)            # the first smallest on the way down
        Z = np.zeros((r, k))
        for j in range(k):
            t = int(tw[j])
            Z[t, j] = 1.0
            for i in range(t - 1, -1, -1):
                Z[i, j] = -e[i] * Z[i + 1, j] / dp[i, j]
            for i in range(t + 1, r):
                Z[i, j] = -e[i - 1] * Z[i - 1, j] / dm[i, j]
    return Z


def orthonormalise(Z):
    """Gram-Schmidt, every vector twice against those before it"""
    U = np.array(Z)
    for j in range(U.shape[1]):
        for _ in range(2):
            if j:
                U[:, j] -= U[:, :j] @ (U[:, :j].T @ U[:, j])
        ss = float(U[:, j] @ U[:, j])
        U[:, j] *= 1.0 / np.sqrt(ss) if ss > 0.0 else 0.0
    return U


def restated_row(X, col):
    """X f64 [m, n], col: the centre's column -> (x^ [m], n_signal), or (None, None) when the rule finds no p"""
    m, n = X.shape
    G, r, q = M.gram(X)
    d, e, V, tau = tridiagonalise_keep(G)
    lam = M.bisect(d, e)
    _, nsig, _, pc = M.rule(lam, q)
    if pc < 0:
        return None, None
    s, cut = int(nsig), r - int(nsig)
    if s == 0:
        return np.zeros(m), 0
    z = X[:, col].copy() if m <= n else np.eye(n)[col]
    for k in range(r - 2):
        z -= tau[k] * float(V[k] @ z) * V[k]
    use_sig = s <= cut
    U = orthonormalise(twisted_vectors(d, e, lam[cut:] if use_sig else lam[:cut]))
    pz = U @ (U.T @ z)
    z = pz if use_sig else z - pz
    for k in range(r - 3, -1, -1):
        z -= tau[k] * float(V[k] @ z) * V[k]
    return (z if m <= n else X @ z), s


def restated(img, mask, w, voxels=None):
    """the restated algorithm over the voxels of mask == 1 (C order; `voxels`: only these indices) -> 'rows' [n_vox, nS] (NaN where not
    eligible or not asked for), 'signal'"""
    img = np.asarray(img)
    sel = np.asarray(mask) == 1
    cs = np.argwhere(sel)
    rows = np.full((len(cs), img.shape[3]), np.nan)
    sig = np.full(len(cs), np.nan)
    for v in (range(len(cs)) if voxels is None else voxels):
        X = M.patch_matrix(img, sel, cs[v], w)
        if 2 * X.shape[1] < w ** 3 or not np.all(np.isfinite(X)):
            continue
        x, s = restated_row(X, centre_column(sel, cs[v], w))
        if x is not None:
            rows[v], sig[v] = x, s
    return {'rows': rows, 'signal': sig}


# ------------------------------------------------------------------ images of high rank
def highrank(shape3, nS, K, sigma, seed, amplitude=100.0, b0=(0,)):
    """every voxel mixes K profiles over the volumes with its own random weights (rank K wherever a patch has K voxels), plus Gaussian
    noise of standard deviation sigma; float32 [X, Y, Z, nS], the clean image as float64, and a mask of ones"""
    rng = np.random.default_rng(seed)
    prof = rng.uniform(0.2, 1.0, size=(K, nS))
    prof[:, list(b0)] = 1.0
    wts = rng.uniform(0.0, 1.0, size=tuple(shape3) + (K,))
    clean = amplitude * (wts @ prof) / K
    img = (clean + sigma * rng.standard_normal(clean.shape)).astype(np.float32)
    return img, clean, np.ones(shape3, dtype=np.uint8)
