"""numpy restatement of the Marchenko-Pastur noise estimator (include/amico_amd.h, "(f0++)"): the cube of a voxel, its columns,
eligibility, the Gram matrix, the rule -- with numpy.linalg.eigvalsh for the eigenvalues -- and, separately, the eigenvalue algorithm the
kernel uses (Householder tridiagonalisation, Sturm-count bisection).  Shared by tests/test_mppca.py and tests/test_gpu_mppca.py."""
import numpy as np

MAX_SIDE = 125
BISECT_STEPS = 56


def cube_start(c, D, w):
    """first voxel of the cube along an axis of length D: clamp(c - h, 0, D - w)"""
    return min(max(c - (w - 1) // 2, 0), D - w)


def patch_matrix(img, sel, centre, w):
    """X f64 [m, n]: the rows are the volumes, the columns the cube's voxels with sel (C order of the cube)"""
    s = [cube_start(int(centre[a]), img.shape[a], w) for a in range(3)]
    cube = (slice(s[0], s[0] + w), slice(s[1], s[1] + w), slice(s[2], s[2] + w))
    return np.ascontiguousarray(img[cube][sel[cube]].astype(np.float64).T)


def gram(X, dtype=np.float64):
    """-> G [r, r] (X X' when m <= n, else X' X), r, q"""
    m, n = X.shape
    Xd = X.astype(dtype)
    G = Xd @ Xd.T if m <= n else Xd.T @ Xd
    return G, min(m, n), max(m, n)


def rule(lam, q):
    """lam ascending [r] -> (sigma, n_signal, margin, p_chosen): margin = the smallest |s2 - s1| / s1 over p; sigma NaN and p_chosen -1
    when no p has s2 < s1"""
    r = len(lam)
    l = np.maximum(lam, 0.0) / q
    S = np.cumsum(l)
    p = np.arange(r)
    gam = (p + 1) / (q - (r - p - 1))
    s1 = S / (p + 1)
    s2 = (l - l[0]) / (4.0 * np.sqrt(gam))
    with np.errstate(divide='ignore', invalid='ignore'):
        margin = float(np.min(np.abs(s2 - s1) / s1)) if np.all(s1 > 0) else 0.0
    ok = np.nonzero(s2 < s1)[0]
    if len(ok) == 0:
        return float('nan'), float('nan'), margin, -1
    pc = int(ok[-1])
    return float(np.sqrt(s1[pc])), float(r - (pc + 1)), margin, pc


# ------------------------------------------------------------------ the kernel's eigenvalue algorithm
def tridiagonalise(G):
    """Householder, unblocked, on the full symmetric matrix: -> d [r], e [r-1].  Step k takes x = A[k+1:, k]: alpha = -sign(x0) |x|,
    v = x - alpha e1, tau2 = 2 / v'v = 1 / (|x|^2 - alpha x0), p = tau2 A v, w = p - (tau2 / 2)(v'p) v, A -= v w' + w v'"""
    A = np.array(G, dtype=np.float64)
    r = A.shape[0]
    d = np.zeros(r)
    e = np.zeros(max(r - 1, 0))
    for k in range(r - 2):
        b = k + 1
        x = A[k, b:].copy()
        sigma2 = float(x @ x)
        d[k] = A[k, k]
        if not sigma2 > 0.0:
            e[k] = 0.0
            continue
        norm = np.sqrt(sigma2)
        alpha = -norm if x[0] >= 0.0 else norm
        e[k] = alpha
        tau2 = 1.0 / (sigma2 - alpha * x[0])
        v = x
        v[0] = x[0] - alpha
        p = tau2 * (A[b:, b:] @ v)
        Kc = 0.5 * tau2 * float(v @ p)
        w_ = p - Kc * v
        A[b:, b:] -= np.outer(v, w_) + np.outer(w_, v)
    if r >= 2:
        d[r - 2] = A[r - 2, r - 2]
        e[r - 2] = A[r - 1, r - 2]
    d[r - 1] = A[r - 1, r - 1]
    return d, e


def bisect(d, e):
    """all eigenvalues of the tridiagonal (d, e), ascending: BISECT_STEPS halvings of the Gershgorin interval widened by 2^-40 of its
    bound; the Sturm count's pivots are kept 2^-104 of that bound away from zero"""
    r = len(d)
    ae = np.abs(e)
    rad = np.zeros(r)
    rad[:-1] += ae
    rad[1:] += ae
    glo, ghi = float(np.min(d - rad)), float(np.max(d + rad))
    bnd = max(abs(glo), abs(ghi))
    pivmin = bnd * 2.0 ** -104
    e2 = e * e
    lo = np.full(r, glo - bnd * 2.0 ** -40)
    hi = np.full(r, ghi + bnd * 2.0 ** -40)
    idx = np.arange(r)
    with np.errstate(divide='ignore', invalid='ignore'):
        for _ in range(BISECT_STEPS):
            mid = 0.5 * (lo + hi)
            qq = d[0] - mid
            qq = np.where(np.abs(qq) < pivmin, -pivmin, qq)
            cnt = (qq < 0).astype(np.int64)
            for i in range(1, r):
                qq = d[i] - mid - e2[i - 1] / qq
                qq = np.where(np.abs(qq) < pivmin, -pivmin, qq)
                cnt += qq < 0
            up = cnt > idx
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
    return 0.5 * (lo + hi)


def eigvals_restated(G):
    return bisect(*tridiagonalise(G))


# ------------------------------------------------------------------ the estimator over an image
def b0_mean(samples):
    """the arithmetic of amx_noise_b0_*: sequential fp64 sum in b0_idx order, one division; NaN without a sample or with a mean <= 0"""
    if len(samples) == 0:
        return float('nan')
    s = np.float64(samples[0])
    for x in samples[1:]:
        s = s + np.float64(x)
    mu = s / np.float64(len(samples))
    return float(mu) if mu > 0 else float('nan')


def estimate(img, mask, b0_idx, w, eigvals=np.linalg.eigvalsh):
    """img f32 [X, Y, Z, nS], mask [X, Y, Z] (== 1 is taken), the voxels in the mask's C order ->
    dict of float64 arrays [n_vox]: 'sigma', 'signal', 'mean', 'ratio', 'margin', 'lam_max', 'r', 'q', 'n', and 'eig' [n_vox, 125]"""
    img = np.asarray(img)
    sel = np.asarray(mask) == 1
    cs = np.argwhere(sel)
    nv = len(cs)
    out = {k: np.full(nv, np.nan) for k in ('sigma', 'signal', 'mean', 'ratio', 'margin', 'lam_max', 'r', 'q', 'n')}
    out['eig'] = np.full((nv, MAX_SIDE), np.nan)
    b0_idx = np.asarray(b0_idx, dtype=np.int64).ravel()
    for v, c in enumerate(cs):
        X = patch_matrix(img, sel, c, w)
        m, n = X.shape
        out['n'][v], out['r'][v], out['q'][v] = n, min(m, n), max(m, n)
        if 2 * n < w ** 3 or not np.all(np.isfinite(X)):
            continue
        G, r, q = gram(X)
        lam = np.sort(eigvals(G))
        sigma, nsig, margin, pc = rule(lam, q)
        if pc < 0:
            continue
        out['eig'][v, :r] = lam
        out['sigma'][v], out['signal'][v], out['margin'][v], out['lam_max'][v] = sigma, nsig, margin, lam[-1]
        out['mean'][v] = b0_mean(img[c[0], c[1], c[2], b0_idx])
        out['ratio'][v] = out['mean'][v] / sigma
    return out


def synthetic(shape3, nS, sigma, seed, amplitude=100.0, components=4, b0=(0,), radius=None):
    """four smooth components plus Gaussian noise of standard deviation sigma, float32 [X, Y, Z, nS], and a spherical mask; the b0
    volumes are the brightest.  radius (in half edges; default 1.05, and 1.3 for volumes of up to 8 voxels a side, which then lose
    little more than their corners: a full 5^3 cube has to fit inside the mask)"""
    if radius is None:
        radius = 1.3 if min(shape3) <= 8 else 1.05
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.linspace(-1.0, 1.0, d) for d in shape3], indexing='ij'), axis=-1)
    maps = np.stack([1.0 + 0.3 * np.sin(2.1 * g[..., 0] + k) * np.cos(1.7 * g[..., 1] - k) + 0.2 * g[..., 2] * (k - 1.5) for k in range(components)],
                    axis=-1)
    prof = rng.uniform(0.2, 1.0, size=(components, nS))
    prof[:, list(b0)] = 1.0
    clean = amplitude * (maps @ prof) / components
    img = (clean + sigma * rng.standard_normal(clean.shape)).astype(np.float32)
    rad = np.sqrt((g ** 2).sum(axis=-1))
    mask = (rad <= radius).astype(np.uint8)
    return img, mask
