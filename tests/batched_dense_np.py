"""numpy restatement of k_batched_big (amico_amd/csrc/amx_batched_big.hip): the solver behind the batched nnls / lasso entry points on
a dictionary marked dense, where the support of a voxel may have any size.

    min_{x >= 0} 1/2 ||y - A x||^2 + lambda1 sum(x) + lambda2 / 2 ||x||^2          (nnls: lambda1 = lambda2 = 0)

in Gram space, H = A'A + lambda2 I, c = A'y - lambda1: block principal pivoting from the K_START best single atoms (all infeasible atoms
change sides while their number keeps falling, K_BACKUP more times after that), then single exchanges, a dense Cholesky factorisation
of H_PP per step.  The single exchanges are Lawson-Hanson's, not Murty's least-index rule: Murty's rule is finite for a positive
definite H only, and with lambda2 = 0 on a dictionary wider than it is tall H is singular -- restated here first with Murty's rule, all
40 voxels of wide_case() ran into the step cap; with Lawson-Hanson's (the atom with the largest dual value per unit norm enters at the
END of the pivot order, atoms leave by the ratio test, the objective never rises) they settle in 40 - 65 steps.  What it has beyond the NODDI kernel it follows (k_noddi_lasso_big):
  1. thresholds relative to the problem: an inactive atom j is infeasible when its dual value exceeds TOL * sqrt(G_jj) * ||y||, a passive
     one when z_j <= 0 -- no absolute constant, so x(c y) = c x(y) (with lambda1 c)
  2. a rank guard: a Cholesky pivot <= PIV * H_jj drops that atom from P for the step (z_j = 0) and switches the voxel to single exchanges;
     the step cap 4 n + 16 ends a voxel that does not settle ('itcap')
  3. a check on the TRUE problem before anything is written: r = y - A_P z from the dictionary, g = A'r - lambda2 z - lambda1; passive
     |g_j| above TOL_P * sqrt(G_jj) * ||y|| -> a refinement solve z += H_PP^-1 g_P (at most REFINE rounds, then 'guard'); an inactive atom with
     a dual above its threshold, or a passive one the refinement turned non-positive, goes back into the pivoting
The input constructors of the tests (CPU and GPU) live here as well, so that both run on the same numbers."""
import numpy as np

K_START, K_BACKUP, REFINE = 32, 3, 3
TOL, TOL_P, PIV = 1e-12, 1e-11, 1e-13


def _cholesky_guarded(H, hd):
    """right-looking Cholesky of H (lower triangle out) that skips a pivot <= PIV * hd[k]: drop[k] = True, row and column k take no part"""
    n = H.shape[0]
    L = np.tril(H).astype(np.float64)
    drop = np.zeros(n, dtype=bool)
    for k in range(n):
        if not L[k, k] > PIV * hd[k]:
            drop[k] = True
            L[k + 1:, k] = 0.0
            continue
        d = np.sqrt(L[k, k])
        L[k, k] = d
        L[k + 1:, k] /= d
        col = L[k + 1:, k]
        L[k + 1:, k + 1:] -= np.tril(np.outer(col, col))
    return L, drop


def _solve(L, drop, b):
    """L w = b, L'z = w on the slots that were not dropped; z = 0 on the dropped ones"""
    n = len(b)
    z = b.astype(np.float64).copy()
    for k in range(n):
        if drop[k]:
            z[k] = 0.0
            continue
        z[k] /= L[k, k]
        z[k + 1:] -= L[k + 1:, k] * z[k]
    for k in range(n - 1, -1, -1):
        if drop[k]:
            z[k] = 0.0
            continue
        z[k] /= L[k, k]
        z[:k] -= L[k, :k] * z[k]
    return z


def solve(A, y, lambda1=0.0, lambda2=0.0, G=None, max_steps=None):
    """-> (x [n], rnorm, info): info = {'steps', 'status' ('ok' | 'itcap' | 'guard'), 'dropped', 'refined', 'single'}"""
    A = np.asarray(A, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    m, n = A.shape
    if G is None:
        G = A.T @ A
    gd = np.diag(G).copy()
    hd = gd + lambda2
    ynorm = np.linalg.norm(y)
    thr = TOL * np.sqrt(gd) * ynorm
    thr_p = TOL_P * np.sqrt(gd) * ynorm
    c = A.T @ y - lambda1
    score = np.where(c > 0.0, c / np.sqrt(np.where(hd > 0, hd, 1.0)), -1.0)
    order = np.lexsort((np.arange(n), -score))                       # by score, ties by index
    inP = np.zeros(n, dtype=bool)
    inP[order[:K_START]] = True
    inP &= score > 0.0
    ninf, backup, single = n + 1, 0, False
    info = {'steps': 0, 'status': 'ok', 'dropped': 0, 'refined': 0, 'single': False}
    z_at, xo = np.zeros(n), np.zeros(n)
    ban = np.zeros(n, dtype=bool)
    plist = np.flatnonzero(inP)
    entered = -1
    r = y.copy()
    step = 0

    def go_single():
        nonlocal single, entered
        single, entered = True, -1
        xo[:] = 0.0
        ban[:] = False
        info['single'] = True

    def ratio_step(P):
        """Lawson-Hanson's step back: from xo towards z until the first passive atom reaches zero; those atoms leave"""
        nonlocal plist, entered
        neg = P[~(z_at[P] > 0.0)]
        ratio = np.where(xo[neg] > 0.0, xo[neg] / (xo[neg] - z_at[neg]), 0.0)
        alpha = ratio.min()
        out = neg[ratio == alpha]
        xo[P] += alpha * (z_at[P] - xo[P])
        xo[out] = 0.0
        inP[out] = False
        if entered >= 0 and entered in out:
            ban[entered] = True                                       # (its dual value said "enter", its coefficient says no: rounding)
        plist = np.array([j for j in plist if inP[j]], dtype=np.int64)
        entered = -1

    while True:
        if step > (4 * n + 16 if max_steps is None else max_steps):
            info['status'] = 'itcap'
            break
        step += 1
        if not single:
            plist = np.flatnonzero(inP)                               # block steps: P in ascending order
        P = plist
        H = G[np.ix_(P, P)] + lambda2 * np.eye(len(P))
        L, drop = _cholesky_guarded(H, hd[P])
        if drop.any():
            # rank guard: the atoms leave P, the voxel goes on by single exchanges (from x = 0 when it was taking block steps)
            info['dropped'] += int(drop.sum())
            if not single:
                go_single()
            else:
                ban[P[drop]] = True
            inP[P[drop]] = False
            plist = P[~drop]
            entered = -1
            continue
        z = _solve(L, drop, c[P])
        z_at[:] = 0.0
        z_at[P] = z
        Z = ~inP
        g = np.full(n, -1.0)
        g[Z] = c[Z] - G[np.ix_(Z, P)] @ z
        if not single:
            bad = np.zeros(n, dtype=bool)
            bad[P] = ~(z_at[P] > 0.0)
            bad[Z] = g[Z] > thr[Z]
        if single or not bad.any():
            if single and not (z_at[P] > 0.0).all():
                ratio_step(P)
                continue
            if single:
                xo[:] = z_at
                if entered >= 0:
                    ban[:] = False
                    entered = -1
            cand = Z & ~ban & (g > thr)
            if not (single and cand.any()):
                # ---- the true problem: residual and gradient from the dictionary itself
                for rnd in range(REFINE + 1):
                    r = y - A[:, P] @ z_at[P]
                    gt = A.T @ r - lambda2 * z_at - lambda1
                    if not (np.abs(gt[P]) > thr_p[P]).any():
                        break
                    if rnd == REFINE:
                        info['status'] = 'guard'
                        break
                    z_at[P] += _solve(L, drop, gt[P])
                    info['refined'] += 1
                if info['status'] == 'guard':
                    break
                g = np.where(Z, gt, -1.0)
                if single:
                    if not (z_at[P] > 0.0).all():
                        ratio_step(P)
                        continue
                    xo[:] = z_at
                    cand = Z & ~ban & (g > thr)
                    if not cand.any():
                        if (Z & (g > thr)).any():
                            info['status'] = 'guard'                  # a banned atom still asks to enter: reported, not hidden
                        break
                else:
                    bad[P] = ~(z_at[P] > 0.0)
                    bad[Z] = g[Z] > thr[Z]
                    if not bad.any():
                        break
        if single:
            # Lawson-Hanson: the atom with the largest dual value per unit norm enters, at the end of the list
            sc = np.where(cand, g / np.sqrt(np.where(gd > 0, gd, 1.0)), -np.inf)
            j = int(np.argmax(sc))
            inP[j] = True
            plist = np.append(plist, j)
            entered = j
            continue
        nbad = int(bad.sum())
        if nbad < ninf:
            ninf, backup = nbad, K_BACKUP
            inP ^= bad
        elif backup > 0:
            backup -= 1
            inP ^= bad
        else:
            go_single()                                               # block steps stall: single exchanges from here, this step's z first
            plist = P                                                 # (the next step factorises the same P again and takes its ratio step)
    info['steps'] = step
    x = np.where(inP & (z_at > 0.0), z_at, 0.0)
    if info['status'] != 'ok':
        r = y - A @ x
    return x, float(np.linalg.norm(r)), info


def kuhn_tucker(A, y, x, lambda1=0.0, lambda2=0.0):
    """(max |g_P|, max g_Z) of x for the problem above, g = A'(y - A x) - lambda2 x - lambda1"""
    g = A.T @ (y - A @ x) - lambda2 * x - lambda1
    P = x > 0
    return float(np.abs(g[P]).max(initial=0.0)), float(g[~P].max(initial=0.0))


# ------------------------------------------------------------------------------------------------------------- the tests' inputs
# item 1 of the GPU tests: (m, n) -> prescribed support sizes, on either side of 16 (main pass), 48 (re-run pass), the LDS factor's limit
SUPPORT_CASES = {
    (200, 60): (5, 16, 17, 20, 40, 48, 49, 50, 55, 59),
    (120, 56): (5, 20, 48, 49, 52, 55),
    (300, 64): (5, 20, 48, 49, 56, 63),
    (260, 200): (5, 20, 48, 49, 64, 65, 100, 150, 176, 177, 190, 199),
    (512, 256): (20, 49, 128, 177, 230, 255),
}
VOXELS_PER_SIZE = 4


def support_problem(m, n, sizes, rng):
    """dictionary [m, n] with m > n and signals whose NNLS optimum is a given support P of k atoms: y = A_P x_P + r, x_P in
    [0.5, 1.5], with a residual r (2 % of the signal: a little noise the optimum cannot absorb) orthogonal to the support's columns
    and with A_j' r equal and negative for every other atom -- then x_P is the NNLS solution itself, with a strict margin
    (the construction of tests/test_gpu_amplitude.py)"""
    A = np.abs(rng.normal(size=(m, n))) + 0.2
    A /= np.linalg.norm(A, axis=0, keepdims=True)
    ys, xs = [], []
    for k in sizes:
        P = np.sort(rng.choice(n, k, replace=False))
        Z = np.setdiff1d(np.arange(n), P)
        x = np.zeros(n)
        x[P] = rng.uniform(0.5, 1.5, k)
        Q, _ = np.linalg.qr(A[:, P])
        B = A[:, Z] - Q @ (Q.T @ A[:, Z])                             # the other atoms off the support's span
        r = -B @ np.linalg.solve(B.T @ B, np.ones(len(Z)))             # A_Z' r = -1, A_P' r = 0
        y = A @ x + 0.02 * np.linalg.norm(A @ x) * r / np.linalg.norm(r)
        ys.append(y)
        xs.append(x)
    return A, np.array(ys), np.array(xs)


def support_case(m, n):
    """-> (A [m, n], y [nv, m], x_true [nv, n], sizes [nv]) of one row of SUPPORT_CASES"""
    sizes = np.repeat(np.array(SUPPORT_CASES[(m, n)]), VOXELS_PER_SIZE)
    A, y, xt = support_problem(m, n, sizes, np.random.default_rng(m * n))
    return A, y, xt, sizes


def elastic_net_case(htable500, n_vox=300):
    """item 3: the six NODDI stage-2 dictionaries (90 x 144, nearly collinear atoms) and the signal mix of
    tests/test_gpu_solvers.py::test_lasso_batched_matches_the_elastic_net -> (A2 [6, 90, 144], y [n_vox, 90], idx [n_vox])"""
    from amico_amd import synthetic as S
    sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, htable500['dirs'])
    ids = np.arange(0, 500, 500 // 6)[:6]
    A = np.stack([np.concatenate([K['wm'][:, d, :].astype(np.float64), K['iso'][None, :].astype(np.float64)], axis=0).T for d in ids])
    dwi = np.asarray(sch.dwi_idx)
    A2 = A[:, dwi, :144] * K['norms'][0][None, None, :]
    rng = np.random.default_rng(5)
    idx = rng.integers(0, A2.shape[0], n_vox).astype(np.int32)
    y = np.abs(A2[idx, :, rng.integers(0, 144, n_vox)] * rng.uniform(0.3, 1.0, (n_vox, 1)) + rng.normal(scale=0.03, size=(n_vox, A2.shape[1])))
    return np.ascontiguousarray(A2), y, idx


ELASTIC_NET_LAMBDAS = ((0.0, 5e-3), (2e-4, 1e-3))


def wide_case():
    """item 4: 60 x 100, lambda2 = 0: every NNLS support has exactly m = 60 atoms and a zero residual -- H_PP is singular as soon as
    a block step gathers more than 60 atoms.  -> (A [60, 100], y [40, 60])"""
    rng = np.random.default_rng(160)
    A = np.abs(rng.normal(size=(60, 100))) + 0.2
    A /= np.linalg.norm(A, axis=0, keepdims=True)
    ys = []
    for _ in range(40):
        x = np.zeros(100)
        x[rng.choice(100, 55, replace=False)] = rng.uniform(0.5, 1.5, 55)
        ys.append(A @ x + 1e-3 * rng.normal(size=60))
    return A, np.array(ys)


SCALES = (2.0 ** -10, 2.0 ** 14)                                      # item 5
