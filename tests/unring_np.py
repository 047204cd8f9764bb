"""Gibbs unringing by local sub-voxel shifts (Kellner et al., MRM 2016; include/amico_amd.h "(f0+++)") in numpy, twice:

  * the oracle -- `unring_slice` / `unring`: np.fft.fft2 for the filter, np.fft.fft / ifft with the phase exp(2 pi i kappa s / n) for the
    shifts, np.roll for the windows;
  * an independent restatement -- `restated_slice`: the shifts as products with circulant matrices built from d_j[t], the filter as
    products with cosine and sine matrices, all in float64, every cosine from an integer reduced modulo its period.

Both return float64; `unring` rounds to float32 once, at the end, and passes a slice with a NaN / Inf sample through."""
import numpy as np

M = 20
MIN_W, MAX_W = 1, 3
SHIFTS = np.concatenate(([0.0], np.arange(1, M + 1) / (2.0 * M), -np.arange(1, M + 1) / (2.0 * M)))
EPS = np.finfo(np.float64).eps
MIN_EXTENT, MAX_EXTENT = 8, 256


def frequencies(n):
    """the signed integer frequencies in np.fft's order; an even n's Nyquist term is marked by 0 in the second array"""
    k = np.fft.fftfreq(n, 1.0 / n)
    keep = np.ones(n)
    if n % 2 == 0:
        keep[n // 2] = 0.0
    return k, keep


def shifted_lines(f):
    """f [..., n] -> g [41, ..., n]: g_j[x] = f(x + s_j) by Fourier interpolation along the last axis; g_0 = f itself"""
    n = f.shape[-1]
    k, keep = frequencies(n)
    F = np.fft.fft(f, axis=-1)
    g = np.empty((len(SHIFTS),) + f.shape)
    g[0] = f
    for j in range(1, len(SHIFTS)):
        g[j] = np.fft.ifft(F * (keep * np.exp(2j * np.pi * k * SHIFTS[j] / n)), axis=-1).real
    return g


def variations(g):
    """g [41, ..., n] -> TV [41, 2, ..., n]: left and right window variation of every pixel for every shift"""
    tv = np.zeros((g.shape[0], 2) + g.shape[1:])
    for t in range(MIN_W, MAX_W + 1):
        tv[:, 0] += np.abs(np.roll(g, t, axis=-1) - np.roll(g, t + 1, axis=-1))          # g[x - t] - g[x - t - 1]
        tv[:, 1] += np.abs(np.roll(g, -t, axis=-1) - np.roll(g, -t - 1, axis=-1))        # g[x + t] - g[x + t + 1]
    return tv


def candidates(g):
    """g [41, ..., n] -> the value every shift would give its pixel, [41, ..., n]"""
    s = SHIFTS.reshape((-1,) + (1,) * (g.ndim - 1))
    a0, a2 = np.roll(g, 1, axis=-1), np.roll(g, -1, axis=-1)
    return np.where(s > 0, (1 - s) * g + s * a0, (1 + s) * g - s * a2)


def pick(g):
    """the map U from the shifted copies: the first strict minimum of the 82 candidates (0, L), (0, R), (1, L), ... wins"""
    tv = variations(g)
    flat = tv.reshape((-1,) + tv.shape[2:])                  # index 2 j + side
    win = np.argmin(flat, axis=0) // 2                       # (argmin returns the first of equal minima)
    return np.take_along_axis(candidates(g), win[None], axis=0)[0]


def U(f):
    """the map U along the last axis of f"""
    return pick(shifted_lines(np.asarray(f, dtype=np.float64)))


def filter_x(n_a, n_b):
    ca = 1.0 + np.cos(2 * np.pi * np.arange(n_a) / n_a)
    cb = 1.0 + np.cos(2 * np.pi * np.arange(n_b) / n_b)
    if n_a % 2 == 0:
        ca[n_a // 2] = 0.0
    if n_b % 2 == 0:
        cb[n_b // 2] = 0.0
    den = ca[:, None] + cb[None, :]
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den == 0.0, 0.5, cb[None, :] / np.where(den == 0.0, 1.0, den))


def split(I):
    """I [n_a, n_b] -> (Ix, Iy): Ix = Re IDFT2(DFT2(I) Gx), Iy = I - Ix"""
    I = np.asarray(I, dtype=np.float64)
    Ix = np.fft.ifft2(np.fft.fft2(I) * filter_x(*I.shape)).real
    return Ix, I - Ix


def unring_slice(I):
    """I [n_a, n_b] (float) -> float64 [n_a, n_b]: U along a of every line of Ix + U along b of every line of Iy"""
    Ix, Iy = split(I)
    return U(Ix.T).T + U(Iy)


def slices_of(img, axes=(0, 1)):
    """img [X, Y, Z] or [X, Y, Z, nS] -> a view [n_a, n_b, n_c, nS] and the function that takes such an array back to img's axes"""
    v = img if img.ndim == 4 else img[..., None]
    a, b = axes
    c = 3 - a - b

    def back(w):
        r = np.moveaxis(w, (0, 1, 2, 3), (a, b, c, 3))
        return np.ascontiguousarray(r if img.ndim == 4 else r[..., 0])
    return np.moveaxis(v, (a, b, c, 3), (0, 1, 2, 3)), back


def unring64(img, axes=(0, 1), one_slice=None):
    """img float32 -> float64 like img: every finite slice through `one_slice` (default: the oracle), before the float32 rounding; a slice
    with a NaN / Inf sample is NaN all over"""
    one_slice = one_slice or unring_slice
    w, back = slices_of(np.asarray(img, dtype=np.float32), axes)
    out = np.full(w.shape, np.nan)
    for z in range(w.shape[2]):
        for s in range(w.shape[3]):
            if np.isfinite(w[:, :, z, s]).all():
                out[:, :, z, s] = one_slice(w[:, :, z, s])
    return back(out)


def unring(img, axes=(0, 1)):
    """img float32 [X, Y, Z] or [X, Y, Z, nS] -> {'image': float32 like img, 'slices', 'passed_through'}"""
    img = np.asarray(img, dtype=np.float32)
    o = unring64(img, axes)
    bad = np.isnan(o)
    w, _ = slices_of(bad, axes)
    res = np.where(bad, img, o.astype(np.float32))
    return {'image': res, 'slices': w.shape[2] * w.shape[3], 'passed_through': int(w[0, 0].sum())}


def margin(slice_max, n_max, c_u):
    """what a float64 evaluation of the definition may differ by from another: 4 C_U n_max eps64 max|slice|"""
    return 4.0 * c_u * n_max * EPS * slice_max


def near_tie_values(I, ia, ib, tau):
    """every value Ux_c + Uy_c' the pixel (ia, ib) of slice I may take from oracle candidates whose TV lies within tau of the minimum"""
    Ix, Iy = split(I)
    sets = []
    for lines, x in ((Ix.T[ib], ia), (Iy[ia], ib)):
        g = shifted_lines(lines[None, :])
        tv = variations(g)[:, :, 0, x].min(axis=1)
        sets.append(candidates(g)[tv <= tv.min() + tau, 0, x])
    return (sets[0][:, None] + sets[1][None, :]).ravel()


def compare(got, img, axes, c_u, ref64=None):
    """got like img (float32 or float64) against the oracle, per pixel: |got - oracle| <= ulp32(|oracle|) + margin, or within that of a
    near-tie value (tau = 12 margin).  -> (worst |got - oracle| / bound over the pixels inside it, pixels that needed the near-tie clause,
    pixels outside both); slices with a NaN / Inf sample are left out"""
    ref64 = unring64(img, axes) if ref64 is None else ref64
    w, _ = slices_of(np.asarray(img, dtype=np.float32), axes)
    r, _ = slices_of(ref64, axes)
    g, _ = slices_of(np.asarray(got), axes)
    n_max = max(w.shape[:2])
    worst, ties, out = 0.0, 0, 0
    for z in range(w.shape[2]):
        for s in range(w.shape[3]):
            I = w[:, :, z, s].astype(np.float64)
            if not np.isfinite(I).all():
                continue
            m = margin(np.abs(I).max(), n_max, c_u)
            bound = np.spacing(np.abs(r[:, :, z, s]).astype(np.float32)).astype(np.float64) + m
            err = np.abs(g[:, :, z, s].astype(np.float64) - r[:, :, z, s])
            ok = err <= bound
            if ok.any():
                worst = max(worst, float((err[ok] / bound[ok]).max()))
            for ia, ib in np.argwhere(~ok):
                vals = near_tie_values(I, ia, ib, 12.0 * m)
                if (np.abs(vals - float(g[ia, ib, z, s])) <= bound[ia, ib]).any():
                    ties += 1
                else:
                    out += 1
    return worst, ties, out


# ------------------------------------------------------------------ the restatement: matrices, no FFT
def shift_table(n):
    """d [41, n]: d_j[t] = (1 / n) sum_kappa cos(2 pi kappa (t + s_j) / n), the argument an integer modulo 40 n (row 0 is the identity)"""
    P = 40 * n
    K = (n - 1) // 2
    kap = np.arange(1, K + 1, dtype=np.int64)
    d = np.zeros((2 * M + 1, n))
    d[0, 0] = 1.0
    for j in range(1, 2 * M + 1):
        jj = j if j <= M else -(j - M)
        q = (40 * np.arange(n, dtype=np.int64) + jj) % P
        m = (kap[None, :] * q[:, None]) % P
        d[j] = (1.0 + 2.0 * np.cos(2 * np.pi * m / P).sum(axis=1)) / n
    return d


def circulant(row):
    n = len(row)
    idx = (np.arange(n)[:, None] - np.arange(n)[None, :]) % n
    return row[idx]


def restated_U(f):
    """the map U along the last axis of f [lines, n] by circulant products"""
    f = np.asarray(f, dtype=np.float64)
    d = shift_table(f.shape[-1])
    g = np.empty((2 * M + 1,) + f.shape)
    g[0] = f
    for j in range(1, 2 * M + 1):
        g[j] = f @ circulant(d[j]).T
    return pick(g)


def dft_tables(n):
    m = (np.arange(n, dtype=np.int64)[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n
    return np.cos(2 * np.pi * m / n), np.sin(2 * np.pi * m / n)


def restated_split(I):
    I = np.asarray(I, dtype=np.float64)
    n_a, n_b = I.shape
    Ca, Sa = dft_tables(n_a)
    Cb, Sb = dft_tables(n_b)
    Pr, Pi = I @ Cb, -(I @ Sb)                               # forward along b
    Qr, Qi = Ca @ Pr + Sa @ Pi, Ca @ Pi - Sa @ Pr            # forward along a
    aa, ab = 1.0 + Ca[:, 1], 1.0 + Cb[:, 1]
    den = aa[:, None] + ab[None, :]
    G = np.where(den == 0.0, 0.5, ab[None, :] / np.where(den == 0.0, 1.0, den))
    Qr, Qi = Qr * G, Qi * G
    Xr, Xi = Ca @ Qr - Sa @ Qi, Ca @ Qi + Sa @ Qr            # inverse along a
    Ix = (Xr @ Cb - Xi @ Sb) / (n_a * n_b)                   # inverse along b, real part
    return Ix, I - Ix


def restated_slice(I):
    Ix, Iy = restated_split(I)
    return restated_U(Ix.T).T + restated_U(Iy)


# ------------------------------------------------------------------ test inputs
def phantom(n_a, n_b, fine=8, noise=0.0, seed=0):
    """ellipses of ~1000 on a grid `fine` times finer, truncated in k-space to [n_a, n_b] -> (ringing image, box-averaged truth), float64"""
    rng = np.random.default_rng(seed)
    Na, Nb = n_a * fine, n_b * fine
    ya, yb = np.meshgrid((np.arange(Na) + 0.5) / Na - 0.5, (np.arange(Nb) + 0.5) / Nb - 0.5, indexing='ij')
    hi = np.zeros((Na, Nb))
    for (ca, cb, ra, rb, v) in [(0.0, 0.0, 0.40, 0.33, 1000.0), (0.02, -0.03, 0.34, 0.27, -400.0), (-0.10, 0.08, 0.09, 0.13, 500.0),
                                (0.13, -0.09, 0.07, 0.05, -450.0)]:
        hi[((ya - ca) / ra) ** 2 + ((yb - cb) / rb) ** 2 <= 1.0] += v
    truth = hi.reshape(n_a, fine, n_b, fine).mean(axis=(1, 3))
    F = np.fft.fftshift(np.fft.fft2(hi))
    a0, b0 = Na // 2 - n_a // 2, Nb // 2 - n_b // 2
    Fc = F[a0:a0 + n_a, b0:b0 + n_b].copy()
    # the low-resolution grid's pixel centres sit (fine - 1) / 2 fine pixels from the fine grid's first: a linear phase
    ka = np.arange(n_a) - n_a // 2
    kb = np.arange(n_b) - n_b // 2
    sh = (fine - 1) / 2.0
    Fc = Fc * np.exp(2j * np.pi * (ka[:, None] * sh / Na + kb[None, :] * sh / Nb))
    low = np.fft.ifft2(np.fft.ifftshift(Fc)).real / fine ** 2
    if noise:
        low = low + noise * rng.standard_normal(low.shape)
    return low, truth


def edge_band(truth, width=6):
    """flat pixels (equal to their four neighbours) within `width` pixels (Chebyshev) of a pixel that is not flat"""
    flat = np.ones(truth.shape, dtype=bool)
    for ax in (0, 1):
        for s in (1, -1):
            flat &= np.abs(truth - np.roll(truth, s, axis=ax)) < 1e-9
    near = np.zeros(truth.shape, dtype=bool)
    edge = ~flat
    for da in range(-width, width + 1):
        for db in range(-width, width + 1):
            near |= np.roll(np.roll(edge, da, axis=0), db, axis=1)
    return flat & near


def noisy_image(shape4, seed):
    """float32 [n_a, n_b, Z, nS]: a noisy phantom per slice (sd 10 on ~1000; the noise keeps the minima generically unique)"""
    n_a, n_b, Z, nS = shape4
    low, _ = phantom(n_a, n_b, fine=4)
    rng = np.random.default_rng(seed)
    img = low[:, :, None, None] * (1.0 + 0.1 * rng.random((1, 1, Z, nS))) + 10.0 * rng.standard_normal(shape4)
    return img.astype(np.float32)


# (n_a, n_b, Z, nS): the in-plane extents at every edge the kernels have -- the smallest, where the windows wrap; odd without a Nyquist term;
# at the tile edges; prime lengths and non-square; the maximum
CASES = [(8, 8, 3, 5), (9, 17, 3, 5), (16, 33, 1, 5), (15, 32, 3, 1), (97, 64, 3, 1), (31, 127, 1, 5), (128, 31, 1, 1), (256, 8, 3, 5),
         (256, 256, 1, 1)]


def case_image(case):
    return noisy_image(case, seed=1000 * case[0] + case[1])
