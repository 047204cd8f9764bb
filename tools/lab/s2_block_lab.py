#!/usr/bin/env python3
"""k_lasso_seed's trip rule, emulated in numpy: how many atoms may enter and leave per trip, and from which pool the entering ones come.

    s2_block_lab.py [n_vox [k [snr]]]          (defaults: 400 voxels, rank 8, SNR 30 -- the benchmark's signal mix)

A trip solves the compressed elastic-net system of the passive set P (M = lambda2 I + S_P S_P', Woodbury form), takes the dual values
t = S'(y~ - M^-1 g) - lambda1 of all atoms, and changes P.  Rules:

  kernel    the rule of the kernel until now: the most negative passive atom leaves and the best atom enters, or -- nothing to
            remove -- the two best atoms enter
  block/N   ALL passive atoms with t <= 0 leave and, in the same trip, the best N of the POOL enter; the pool is what the scan holds in
            registers anyway: the two largest dual values of each row class j mod 4 (a lane's elements are the atoms 16 mt + 4 rr + q)
  groups/N  the same with the pool "the largest of each of the 8 groups (j mod 4, tile parity)": one running maximum per group
  true/N    the same with the N largest dual values of all atoms (what a full sort would give)
  class     all t <= 0 leave, the best of each row class enters (up to 4)
  one/N     ONE atom leaves (the most negative), the best N of the pool enter in the same trip

Columns: share of voxels that end on exactly the support of the exact LASSO solution of the compressed problem's parent (scipy NNLS on
the augmented system), trips per voxel (mean / 95th percentile / maximum; the cap is 300), changes of the set per voxel.
"""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from amico_amd import synthetic as S          # noqa: E402

LAM1, LAM2, TOL, CAP = 0.5, 1e-3, 1e-9, 300


def rrqr(A, k):
    """the first k directions of the pivoted Gram-Schmidt basis k_build_basis makes"""
    R = A.copy(); Q = []
    for _ in range(k):
        nr = (R * R).sum(0); j = int(np.argmax(nr)); q = R[:, j] / np.sqrt(nr[j])
        for _ in range(2):
            for p in Q:
                q = q - p * (p @ q)
            q /= np.linalg.norm(q)
        Q.append(q); R = R - np.outer(q, q @ R)
    return np.array(Q).T


def lasso_exact(A2, y2, lam1=LAM1, lam2=LAM2):
    from scipy.optimize import nnls
    n = A2.shape[1]
    Aa = np.vstack([A2, np.sqrt(lam2) * np.eye(n)]); ya = np.concatenate([y2, np.zeros(n)])
    cvec = Aa @ np.linalg.solve(Aa.T @ Aa, lam1 * np.ones(n))
    return nnls(Aa, ya - cvec, maxiter=20000)[0]


def pool_of(cand, kind):
    """atoms of the pool, best first"""
    n = len(cand)
    if kind == 'true':
        pool = list(np.argsort(-cand))
    elif kind == 'block':           # top two of each class j mod 4
        pool = [j for q in range(4) for j in np.arange(q, n, 4)[np.argsort(-cand[q::4])[:2]]]
    elif kind == 'groups':          # top one of each (j mod 4, tile parity)
        pool = []
        for q in range(4):
            for par in range(2):
                idx = np.array([j for j in range(q, n, 4) if ((j >> 4) & 1) == par])
                pool.append(idx[np.argmax(cand[idx])])
    elif kind == 'class':
        pool = [np.arange(q, n, 4)[np.argmax(cand[q::4])] for q in range(4)]
    else:
        raise ValueError(kind)
    return sorted((j for j in pool if cand[j] > TOL), key=lambda j: -cand[j])


def trips(Sk, yt, rule, lam1=LAM1, lam2=LAM2, max_atoms=None, cap=CAP):
    """(P, trips, changes) of one voxel; rule = ('kernel',) or (pool kind, N entering, all_leave)"""
    kk, n = Sk.shape
    P = np.zeros(n, bool); nt = 0; ch = 0
    for _ in range(cap):
        nt += 1
        SP = Sk[:, P]
        M = lam2 * np.eye(kk) + SP @ SP.T
        w = np.linalg.solve(M, SP @ (SP.T @ yt - lam1))
        t = Sk.T @ (yt - w) - lam1
        cand = np.where(~P, t, -np.inf)
        neg = np.flatnonzero(P & (t <= 0))
        if rule[0] == 'kernel':
            order = np.argsort(-cand)
            if len(neg):
                P[neg[np.argmin(t[neg])]] = False; ch += 1
                ent = [j for j in order[:1] if cand[j] > TOL]
            else:
                ent = [j for j in order[:2] if cand[j] > TOL]
                if not ent:
                    break
        else:
            kind, n_in, all_leave = rule
            ent = pool_of(cand, kind)[:n_in]
            if not len(neg) and not ent:
                break
            if not all_leave and len(neg):
                neg = neg[[np.argmin(t[neg])]]
            P[neg] = False; ch += len(neg)
        if max_atoms is not None:
            ent = ent[:max(0, max_atoms - int(P.sum()))]
        P[ent] = True; ch += len(ent)
    return P, nt, ch


RULES = {
    'kernel (2 enter / 1 leaves + 1 enters)': ('kernel',),
    'all <= 0 leave + best 4 of the pool': ('block', 4, True),
    'all <= 0 leave + best 3 of the pool': ('block', 3, True),
    'all <= 0 leave + best 6 of the pool': ('block', 6, True),
    'all <= 0 leave + best 4 of 8 group maxima': ('groups', 4, True),
    'all <= 0 leave + true best 4': ('true', 4, True),
    'all <= 0 leave + best of each class (4)': ('class', 4, True),
    'ONE leaves + best 4 of the pool': ('block', 4, False),
}


def problems(n_vox, k, snr, seed=3):
    """(S2, y2~, exact support) of n_vox benchmark-mix voxels"""
    from scipy.optimize import nnls
    dirs = S.fibonacci_hemisphere(500); ht = S.build_htable(dirs); sch = S.make_scheme(seed=0)
    K = S.noddi_kernels(sch, dirs)
    y, d = S.noddi_signals(n_vox, K, ht, sch, seed=seed, snr=snr)
    lut = S.lut_indices(d, ht); wm = K['wm']; iso = K['iso'].astype(np.float64)
    dwi = np.asarray(sch.dwi_idx); norms = K['norms'][0]
    cache = {}
    for v in range(n_vox):
        if lut[v] not in cache:
            A = np.concatenate([wm[:, lut[v], :].astype(np.float64).T, iso[:, None]], axis=1)
            A2 = A[dwi][:, :wm.shape[0]] * norms[None, :]
            U2 = rrqr(A2, k); cache[lut[v]] = (A, A2, U2, U2.T @ A2)
        A, A2, U2, S2 = cache[lut[v]]
        x1, _ = nnls(A, y[v], maxiter=5000)
        y2 = np.maximum(y[v][dwi] - x1[-1] * iso[dwi], 0.0)
        yield S2, U2.T @ y2, lasso_exact(A2, y2) > 0


def main():
    n_vox = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    snr = float(sys.argv[3]) if len(sys.argv) > 3 else 30.0
    res = {r: [] for r in RULES}
    for S2, yt, P2 in problems(n_vox, k, snr):
        for name, rule in RULES.items():
            P, nt, ch = trips(S2, yt, rule)
            res[name].append(((P == P2).all(), nt, ch))
    print('voxels %d, rank %d, SNR %g' % (n_vox, k, snr))
    for name, r in res.items():
        a = np.array(r, float)
        print('%-44s exact %5.1f%%  trips mean %.2f p95 %.0f max %.0f  changes %.1f' % (
            name, 100 * a[:, 0].mean(), a[:, 1].mean(), np.percentile(a[:, 1], 95), a[:, 1].max(), a[:, 2].mean()))


if __name__ == '__main__':
    main()
