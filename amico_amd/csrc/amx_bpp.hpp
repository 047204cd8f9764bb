// amx_bpp.hpp -- block principal pivoting on a packed Cholesky factor, one WORKGROUP of 256 threads per voxel: the loop k_batched_big
// (amx_batched_big.hip) and k_enet_big (amx_enet_big.hip) share.
//     min_{x >= 0} 1/2 ||y - A x||^2 + lambda1 sum(x) + lambda2/2 ||x||^2
// in Gram space, H = G + lambda2 I from a Gram table in HBM, c = A'y - lambda1 from the tile where it lies (float64 or float32).  All
// infeasible atoms change sides while their number keeps falling (then kBackup more times), a dense Cholesky factorisation of H_PP per step
// -- packed, in LDS while the passive set fits (`lcap` atoms: what the 160 KB leave beside the vectors), in a global block per workgroup beyond.
//   1. thresholds relative to the problem: an inactive atom j is infeasible when its dual value exceeds kTol sqrt(G_jj) ||y||, a passive one
//      when z_j <= 0.  No absolute constant: x(c y) = c x(y), for lasso with lambda1 c.
//   2. a rank guard (ASPACE refines it for the single exchanges: kSmall below).  With lambda2 = 0, H_PP may be singular (a block step gathers more atoms than samples, or dependent ones): a pivot
//      <= kPiv H_jj drops that atom from P and the voxel goes on by SINGLE exchanges from x = 0.  Those are Lawson-Hanson's, not Murty's
//      least-index rule: Murty's is finite for a positive definite H only (restated in numpy, tests/batched_dense_np.py, every voxel of a 60 x 100
//      dictionary ran into the step cap with it).  The atom with the largest dual value per unit norm enters at the END of the pivot order -- so
//      only the entering atom can fail the pivot test --, atoms leave by the ratio test, the objective never rises.  A voxel whose block steps
//      stall takes the same road.  The step cap 4 n + 16 ends a voxel that does not settle: kIterCap, never a hang.
//   3. a check on the TRUE problem before anything is written: r = y - A_P z and g = A'r - lambda2 z - lambda1 from the tile.  A passive |g_j|
//      above kTolP sqrt(G_jj) ||y|| asks for a refinement solve z += H_PP^-1 g_P (at most kRefine rounds, then kGuardOuter); an inactive atom
//      with a dual above its threshold, or a passive one the refinement turned non-positive, sends the voxel back into the pivoting.
// Every sum runs in an order fixed by the shape alone: the same signal gives the same bits wherever the voxel stands in a call.
#pragma once
#include "amx_solver.hpp"

namespace amx {
namespace bpp {

constexpr int kStart = 32, kBackup = 3, kRefine = 3;
constexpr double kTol = 1e-12, kTolP = 1e-11, kPiv = 1e-13;
// ASPACE (k_enet_big): a pivot of the single exchanges below kSmall H_jj is evaluated again in A-space, and dropped at kPivA H_jj only.
// The Gram-space pivot H_jj - |l|^2 carries an error of ~1e-15 H_jj, so at 1e-13 H_jj -- an atom within 3e-7 of the span of the passive ones --
// it has one digit, and kPiv drops the atom.  On the coherent dictionaries of the models (255 zeppelins, 21 volumes, lambda2 = 0) that atom may be
// the one the optimum needs: its dual value a_j'r = d'r is up to 3e-7 |a_j| |r|, 1e-8 of the signal, and a voxel that bans it ends at the guard
// with that much left (33 of 365 hard voxels).  With w = L^-T l (one back substitution) the pivot is |a_j - A_P w|^2 + lambda2 (1 + |w|^2) from the
// tile (tests/big_np.py: pivots_of_last_atom).  kPivA = kTol^2: an atom nearer to the span than that cannot have a dual value above its threshold
// kTol sqrt(G_jj) |y|.  What the evaluation itself can tell is less when the slots before are ill-conditioned too: w comes from the Gram-space
// factor, whose condition is 1 / rho with rho the smallest pivot ratio L_ss^2 / H_ss before this slot, and an error of eps / rho in w along a
// direction A_P shrinks by sqrt(rho) leaves eps (1 + |w|_1) / sqrt(rho) in the difference: a pivot below kFloor (1 + |w|_1)^2 / rho H_jj,
// kFloor = (32 eps)^2, is noise and drops the atom (tests/test_big_dictionaries.py: zeppelin 106 of 255 behind zeppelins 100, 102 .. 110 -- itself
// among them, true pivot 0 -- evaluates to 1.6e-17 H_jj, floor 1e-13 H_jj; zeppelin 105 behind 100, 110, 120: true 4.473e-15 H_jj, Gram space
// 4.263e-15, A-space 4.473e-15, floor 2e-20).
constexpr double kSmall = 1e-6, kPivA = 1e-24, kFloor = 1024.0 * 2.220446049250313e-16 * 2.220446049250313e-16;

// deterministic minimum over the workgroup
__device__ __forceinline__ double block_min(double v, double *part, int tid)
{
    __syncthreads();
    part[tid] = v;
    __syncthreads();
    for (int w = 256 / 2; w > 0; w >>= 1) {
        if (tid < w) part[tid] = part[tid + w] < part[tid] ? part[tid + w] : part[tid];
        __syncthreads();
    }
    const double t = part[0];
    __syncthreads();
    return t;
}

__device__ __forceinline__ int tri_at(int r, int s) { return r * (r + 1) / 2 + s; }      // (<= 256 atoms: 32 896 entries)

// deterministic sum over the workgroup (the same tree whatever the data: the host and device forms agree bit for bit)
__device__ __forceinline__ double block_sum(double v, double *part, int tid)
{
    __syncthreads();
    part[tid] = v;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    const double t = part[0];
    __syncthreads();
    return t;
}

// out[j] = sum_i A[i][j] v[i], j < n: the threads over (row part, atom) so that a wavefront reads consecutive atoms of one row
template <typename AT>
__device__ __forceinline__ void tile_t_times(const AT *__restrict__ At, int ldA, int m, int n, const double *v, double *out, double *part, int tid)
{
    const int parts = kThreads / n > 0 ? kThreads / n : 1;           // (n <= 256)
    __syncthreads();
    if (tid < parts * n) {
        const int j = tid % n, p = tid / n;
        double acc = 0.0;
        for (int i = p; i < m; i += parts) acc += (double)At[(size_t)i * ldA + j] * v[i];
        part[tid] = acc;
    }
    __syncthreads();
    if (tid < n) {
        double acc = part[tid];
        for (int p = 1; p < parts; p++) acc += part[p * n + tid];
        out[tid] = acc;
    }
    __syncthreads();
}

// r = y - A x over the atoms of plist (x in atom order; clip: only its positive entries): 16 threads share a row
template <typename AT>
__device__ __forceinline__ void tile_residual(const AT *__restrict__ At, int ldA, int m, const int *plist, int np, const double *x, bool clip,
                                              const double *y, double *r, int tid)
{
    __syncthreads();
    for (int i0 = 0; i0 < m; i0 += 16) {
        const int i = i0 + (tid >> 4);
        double acc = 0.0;
        if (i < m)
            for (int s = tid & 15; s < np; s += 16) {
                const int j = plist[s];
                const double xj = x[j];
                if (!clip || xj > 0.0) acc += (double)At[(size_t)i * ldA + j] * xj;
            }
        acc += __shfl_xor(acc, 8, 16);
        acc += __shfl_xor(acc, 4, 16);
        acc += __shfl_xor(acc, 2, 16);
        acc += __shfl_xor(acc, 1, 16);
        if ((tid & 15) == 0 && i < m) r[i] = y[i] - acc;
    }
    __syncthreads();
}

// Cholesky in place, right-looking, packed lower triangle; a pivot <= kPiv H_jj is skipped (drp[k] = 1, *ndrop counts them; its column is cleared).
// col [np] (LDS) holds the scaled column of the pivot: the trailing update reads both of its factors from there -- contiguous, and from LDS
// also when the factor lies in its global block -- instead of gathering them from the packed triangle
// ASPACE: see kSmall; aspace = this factorisation is a single exchange's; wv [np] and part [256] are LDS scratch
template <bool ASPACE = false, typename AT = double>
__device__ __forceinline__ void factor_guarded(double *L, int np, const int *plist, const double *hd, int *drp, int *ndrop, double *col, int tid,
                                               bool aspace = false, const AT *__restrict__ At = nullptr, int ldA = 0, int m = 0, double lam2 = 0.0,
                                               double *wv = nullptr, double *part = nullptr)
{
    __syncthreads();
    for (int k = 0; k < np; k++) {
        double dk = L[tri_at(k, k)];
        bool ok = dk > kPiv * hd[plist[k]];
        __syncthreads();                                     // (every thread has read the pivot)
        if constexpr (ASPACE) {
            if (aspace && *ndrop == 0 && !(dk > kSmall * hd[plist[k]])) {      // (uniform: LDS values every thread reads alike)
                // w = L^-T l over the k slots before this one (none of them dropped), column oriented like tri_solve
                for (int r = tid; r < k; r += kThreads) wv[r] = L[tri_at(k, r)];
                __syncthreads();
                for (int s = k - 1; s >= 0; s--) {
                    const double ws = wv[s] / L[tri_at(s, s)];
                    __syncthreads();
                    if (tid == 0) wv[s] = ws;
                    for (int r = tid; r < s; r += kThreads) wv[r] -= L[tri_at(s, r)] * ws;
                    __syncthreads();
                }
                // |a_k - A_P w|^2 from the tile, 16 threads to a row; + lambda2 (1 + |w|^2)
                const int jk = plist[k];
                double dd = 0.0;
                for (int i0 = 0; i0 < m; i0 += 16) {
                    const int i = i0 + (tid >> 4);
                    double acc = 0.0;
                    if (i < m)
                        for (int s = tid & 15; s < k; s += 16) acc += (double)At[(size_t)i * ldA + plist[s]] * wv[s];
                    acc += __shfl_xor(acc, 8, 16);
                    acc += __shfl_xor(acc, 4, 16);
                    acc += __shfl_xor(acc, 2, 16);
                    acc += __shfl_xor(acc, 1, 16);
                    if ((tid & 15) == 0 && i < m) { const double d = (double)At[(size_t)i * ldA + jk] - acc; dd += d * d; }
                }
                double ww = 0.0, w1 = 0.0, rho = 1.0;
                for (int r = tid; r < k; r += kThreads) {
                    const double lrr = L[tri_at(r, r)], q = lrr * lrr / hd[plist[r]];
                    ww += wv[r] * wv[r]; w1 += fabs(wv[r]);
                    rho = q < rho ? q : rho;
                }
                dk = block_sum(dd, part, tid) + lam2 * (1.0 + block_sum(ww, part, tid));
                w1 = 1.0 + block_sum(w1, part, tid);
                rho = block_min(rho, part, tid);
                const double fl = kFloor * w1 * w1 / rho;
                ok = dk > (fl > kPivA ? fl : kPivA) * hd[jk];
                if (tid == 0) L[tri_at(k, k)] = dk;
                __syncthreads();
            }
        }
        if (!ok) {
            for (int r = k + 1 + tid; r < np; r += kThreads) L[tri_at(r, k)] = 0.0;
            if (tid == 0) { drp[k] = 1; *ndrop += 1; }
            __syncthreads();
            continue;
        }
        const double d = sqrt(dk), di = 1.0 / d;
        for (int r = k + tid; r < np; r += kThreads) {
            const double v = (r == k) ? d : L[tri_at(r, k)] * di;
            L[tri_at(r, k)] = v; col[r] = v;
        }
        __syncthreads();
        // (16 x 16 threads over the trailing triangle: amx_big.hip measured it at three times a thread per row)
        for (int r = k + 1 + (tid >> 4); r < np; r += 16) {
            const double lrk = col[r];
            for (int s = k + 1 + (tid & 15); s <= r; s += 16) L[tri_at(r, s)] -= lrk * col[s];
        }
        __syncthreads();
    }
}

// L w = b, L'z = w in place (column oriented: one step per pivot); no dropped pivot in L
__device__ __forceinline__ void tri_solve(const double *L, int np, double *zv, int tid)
{
    __syncthreads();
    for (int k = 0; k < np; k++) {
        const double wk = zv[k] / L[tri_at(k, k)];
        __syncthreads();
        if (tid == 0) zv[k] = wk;
        for (int r = k + 1 + tid; r < np; r += kThreads) zv[r] -= L[tri_at(r, k)] * wk;
        __syncthreads();
    }
    for (int k = np - 1; k >= 0; k--) {
        const double zk = zv[k] / L[tri_at(k, k)];
        __syncthreads();
        if (tid == 0) zv[k] = zk;
        for (int r = tid; r < k; r += kThreads) zv[r] -= L[tri_at(k, r)] * zk;
        __syncthreads();
    }
}

// plist keeps the atoms still in P, in the order it holds them (tmp: n ints); *np_out = how many
__device__ __forceinline__ void compact_plist(int *plist, int np, const int *inP, int *tmp, int *np_out, int tid)
{
    __syncthreads();
    for (int r = tid; r < np; r += kThreads) {
        const int j = plist[r];
        if (inP[j]) {
            int pos = 0;
            for (int s = 0; s < r; s++) pos += inP[plist[s]];
            tmp[pos] = j;
        }
    }
    if (tid == 0) { int c2 = 0; for (int s = 0; s < np; s++) c2 += inP[plist[s]]; *np_out = c2; }
    __syncthreads();
    const int c2 = *np_out;
    for (int r = tid; r < c2; r += kThreads) plist[r] = tmp[r];
    __syncthreads();
}

// the workgroup's vectors in LDS, carved from one block of vec_bytes(m, n) bytes; the packed factor of <= lcap atoms lies behind them
struct Work {
    double *yv;       // [m] signal (the caller fills it, and rv with a copy)
    double *rv;       // [m] true residual
    double *cv;       // [n] c_j = a_j'y - lambda1
    double *zv;       // [n] right-hand side / solution in slot order
    double *zat;      // [n] solution in atom order
    double *xo;       // [n] the feasible point of the single exchanges
    double *gv;       // [n] dual values of the inactive atoms
    double *gtv;      // [n] gradient of the true problem
    double *thr;      // [n] kTol sqrt(G_jj) ||y||
    double *hd;       // [n] H_jj
    double *sgd;      // [n] sqrt(G_jj)
    double *part;     // [256] partial sums, scores, ratios
    double *dsc;      // [2] scalars
    int *plist;       // [n] atoms of P in pivot order
    int *inP;         // [n] 1 = passive
    int *bad;         // [n] 1 = infeasible this step; scratch of compact_plist
    int *ban;         // [n] 1 = may not enter until x moves
    int *drp;         // [n] 1 = slot dropped by the rank guard
    int *shi;         // [16] scalars: 0 np, 1 n_bad, 2 entering atom, 3 dropped pivots, 4 non-finite, 5 passive z <= 0, 6 |g_P| above tolerance, 7 a banned atom asks to enter
    double *Ll;       // packed lower triangle, <= lcap atoms
};

// (kThreads, vec_bytes: amx_sizes.hpp)
__device__ __forceinline__ Work carve(unsigned char *smem, int m, int n)
{
    const int mp = (m + 1) & ~1, npd = (n + 1) & ~1, n4 = (n + 3) & ~3;
    Work w;
    w.yv = reinterpret_cast<double *>(smem);
    w.rv = w.yv + mp;
    w.cv = w.rv + mp;
    w.zv = w.cv + npd;
    w.zat = w.zv + npd;
    w.xo = w.zat + npd;
    w.gv = w.xo + npd;
    w.gtv = w.gv + npd;
    w.thr = w.gtv + npd;
    w.hd = w.thr + npd;
    w.sgd = w.hd + npd;
    w.part = w.sgd + npd;
    w.dsc = w.part + kThreads;
    w.plist = reinterpret_cast<int *>(w.dsc + 2);
    w.inP = w.plist + n4;
    w.bad = w.inP + n4;
    w.ban = w.bad + n4;
    w.drp = w.ban + n4;
    w.shi = w.drp + n4;
    w.Ll = reinterpret_cast<double *>(w.shi + 16);
    return w;
}

// One voxel.  In: yv = rv = the signal, ynorm = ||y||, shi[] zeroed.  Out: zat (atom order; x_j = zat_j where inP_j and zat_j > 0, else 0),
// rv = y - A x of exactly that x, plist[0 .. shi[0]) = the atoms of P; the status (kSolved, kIterCap, a guard) and the steps taken.
// full_start: P starts as every atom (a strong ridge without lambda1: a dense optimum); else as the kStart atoms that fit the signal best on
// their own (c_j / sqrt(H_jj), c_j > 0).  Lg: the workgroup's global factor block for passive sets beyond lcap atoms (or Ll when lcap >= n).
template <typename AT, bool ASPACE = false>
__device__ __forceinline__ int solve(const Work &w, const AT *__restrict__ At, int ldA, int m, int n, const double *__restrict__ G, int ldG,
                                     double lam1, double lam2, double ynorm, int lcap, double *Lg, bool full_start, int *steps_out, int tid)
{
    constexpr int nt = kThreads;
    double *yv = w.yv, *rv = w.rv, *cv = w.cv, *zv = w.zv, *zat = w.zat, *xo = w.xo, *gv = w.gv, *gtv = w.gtv, *thr = w.thr, *hd = w.hd, *sgd = w.sgd;
    double *part = w.part, *dsc = w.dsc, *Ll = w.Ll;
    int *plist = w.plist, *inP = w.inP, *bad = w.bad, *ban = w.ban, *drp = w.drp, *shi = w.shi;
    // ---- c, thresholds; the first passive set
    tile_t_times(At, ldA, m, n, yv, cv, part, tid);
    for (int j = tid; j < n; j += nt) {
        const double gjj = G[(size_t)j * ldG + j];
        const double cj = cv[j] - lam1;
        cv[j] = cj;
        sgd[j] = sqrt(gjj); hd[j] = gjj + lam2; thr[j] = kTol * sqrt(gjj) * ynorm;
        zat[j] = (cj > 0.0 && gjj + lam2 > 0.0) ? cj / sqrt(gjj + lam2) : -1.0;       // (score; zat is free until the first solve)
        xo[j] = 0.0; ban[j] = 0;
    }
    __syncthreads();
    for (int j = tid; j < n; j += nt) {
        const double sj = zat[j];
        int rank = 0;
        if (!full_start)
            for (int k = 0; k < n; k++) rank += (zat[k] > sj || (zat[k] == sj && k < j)) ? 1 : 0;
        inP[j] = full_start ? 1 : ((sj > 0.0 && rank < kStart) ? 1 : 0);
    }
    __syncthreads();
    int ninf = n + 1, backup = 0, status = kSolved, steps_done = 0, entered = -1;
    bool single = false;
    for (int step = 0;; ++step) {
        if (step > 4 * n + 16) { status = kIterCap; break; }
        steps_done = step + 1;
        // ---- P: in ascending order for a block step; the single exchanges keep their own order (the entering atom last)
        if (!single) {
            for (int j = tid; j < n; j += nt) {
                if (inP[j]) {
                    int r = 0;
                    for (int k = 0; k < j; k++) r += inP[k];
                    plist[r] = j;
                }
            }
            if (tid == 0) { int c2 = 0; for (int k = 0; k < n; k++) c2 += inP[k]; shi[0] = c2; }
        }
        if (tid == 0) { shi[1] = 0; shi[2] = -1; shi[3] = 0; shi[5] = 0; shi[6] = 0; shi[7] = 0; }
        __syncthreads();
        const int np = shi[0];
        const bool in_lds = np <= lcap;
        // ---- H_PP (packed lower triangle), the right-hand side
        for (int r = tid >> 4; r < np; r += 16) {
            const int pr = plist[r];
            const double *Gr = G + (size_t)pr * ldG;
            for (int s = tid & 15; s <= r; s += 16) {
                const double h = Gr[plist[s]] + (s == r ? lam2 : 0.0);
                if (in_lds) Ll[tri_at(r, s)] = h; else Lg[tri_at(r, s)] = h;
            }
        }
        for (int r = tid; r < np; r += nt) { zv[r] = cv[plist[r]]; drp[r] = 0; }
        // (gtv is free until the true problem's pass, gv and part until the dual values are made)
        if (in_lds) factor_guarded<ASPACE, AT>(Ll, np, plist, hd, drp, &shi[3], gtv, tid, single, At, ldA, m, lam2, gv, part);
        else factor_guarded<ASPACE, AT>(Lg, np, plist, hd, drp, &shi[3], gtv, tid, single, At, ldA, m, lam2, gv, part);
        __syncthreads();
        if (shi[3] > 0) {
            // rank guard: those atoms leave P; single exchanges from here (from x = 0 when the voxel was taking block steps)
            for (int r = tid; r < np; r += nt)
                if (drp[r]) { inP[plist[r]] = 0; if (single) ban[plist[r]] = 1; }
            if (!single) { for (int j = tid; j < n; j += nt) { xo[j] = 0.0; ban[j] = 0; } }
            single = true; entered = -1;
            compact_plist(plist, np, inP, bad, &shi[0], tid);
            continue;
        }
        if (in_lds) tri_solve(Ll, np, zv, tid); else tri_solve(Lg, np, zv, tid);
        for (int j = tid; j < n; j += nt) zat[j] = 0.0;
        __syncthreads();
        for (int r = tid; r < np; r += nt) zat[plist[r]] = zv[r];
        __syncthreads();
        // ---- dual values of the inactive atoms in Gram space: g_j = c_j - sum_s H_js z_s
        for (int j = tid; j < n; j += nt) {
            double g = -1.0;
            if (!inP[j]) {
                const double *Gj = G + (size_t)j * ldG;
                double acc = 0.0;
                for (int r = 0; r < np; r++) acc += Gj[plist[r]] * zv[r];
                g = cv[j] - acc;
            }
            gv[j] = g;
        }
        __syncthreads();
        // ---- decide: pass 0 on the Gram-space numbers; if they say "optimum", pass 1 on the true problem's
        bool finished = false;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1) {
                for (int rnd = 0;; ++rnd) {
                    tile_residual(At, ldA, m, plist, np, zat, false, yv, rv, tid);
                    tile_t_times(At, ldA, m, n, rv, gtv, part, tid);
                    if (tid == 0) shi[6] = 0;
                    __syncthreads();
                    for (int j = tid; j < n; j += nt) gtv[j] = gtv[j] - lam2 * zat[j] - lam1;
                    __syncthreads();
                    for (int r = tid; r < np; r += nt)
                        if (fabs(gtv[plist[r]]) > (kTolP / kTol) * thr[plist[r]]) shi[6] = 1;
                    __syncthreads();
                    if (!shi[6]) break;
                    if (rnd == kRefine) { status = kGuardOuter; break; }
                    for (int r = tid; r < np; r += nt) zv[r] = gtv[plist[r]];
                    if (in_lds) tri_solve(Ll, np, zv, tid); else tri_solve(Lg, np, zv, tid);
                    for (int r = tid; r < np; r += nt) zat[plist[r]] += zv[r];
                    __syncthreads();
                }
                if (status != kSolved) { finished = true; break; }
                for (int j = tid; j < n; j += nt) gv[j] = inP[j] ? -1.0 : gtv[j];
                if (tid == 0) { shi[1] = 0; shi[2] = -1; shi[5] = 0; shi[7] = 0; }
                __syncthreads();
            }
            if (!single) {
                for (int j = tid; j < n; j += nt) {
                    const bool v = inP[j] ? !(zat[j] > 0.0) : gv[j] > thr[j];
                    bad[j] = v ? 1 : 0;
                    if (v) atomicAdd(&shi[1], 1);
                }
                __syncthreads();
                const int nbad = shi[1];
                if (nbad == 0) {
                    if (pass == 0) continue;
                    finished = true;
                    break;
                }
                if (nbad < ninf) { ninf = nbad; backup = kBackup; }
                else if (backup > 0) backup--;
                else {                                            // the block steps stall: single exchanges, this P first
                    single = true; entered = -1;
                    for (int j = tid; j < n; j += nt) { xo[j] = 0.0; ban[j] = 0; }
                    __syncthreads();
                    break;
                }
                for (int j = tid; j < n; j += nt)
                    if (bad[j]) inP[j] ^= 1;
                __syncthreads();
                break;
            }
            // ---- single exchanges (Lawson-Hanson): the ratio test first
            for (int r = tid; r < np; r += nt) {
                const int j = plist[r];
                double ratio = 2.0;
                if (!(zat[j] > 0.0)) { ratio = xo[j] > 0.0 ? xo[j] / (xo[j] - zat[j]) : 0.0; shi[5] = 1; }
                part[r] = ratio;
            }
            __syncthreads();
            if (shi[5]) {
                if (tid == 0) { double al = 2.0; for (int r = 0; r < np; r++) al = part[r] < al ? part[r] : al; dsc[0] = al; }
                __syncthreads();
                const double alpha = dsc[0];
                for (int r = tid; r < np; r += nt) {
                    const int j = plist[r];
                    xo[j] += alpha * (zat[j] - xo[j]);
                    if (part[r] == alpha) { xo[j] = 0.0; inP[j] = 0; if (j == entered) ban[j] = 1; }      // (its dual value said "enter", its coefficient says no: rounding)
                }
                entered = -1;
                compact_plist(plist, np, inP, bad, &shi[0], tid);
                break;
            }
            for (int j = tid; j < n; j += nt) { xo[j] = zat[j]; if (entered >= 0) ban[j] = 0; }
            entered = -1;
            __syncthreads();
            // the atom with the largest dual value per unit norm enters, at the end of the pivot order
            for (int j = tid; j < n; j += nt) {
                const bool over = !inP[j] && gv[j] > thr[j];
                part[j] = (over && !ban[j]) ? gv[j] / sgd[j] : -1.0;
                if (over && ban[j]) shi[7] = 1;
            }
            __syncthreads();
            for (int j = tid; j < n; j += nt) {
                const double sj = part[j];
                if (sj > 0.0) {
                    bool best = true;
                    for (int k = 0; k < n; k++) best = best && !(part[k] > sj || (part[k] == sj && k < j));
                    if (best) shi[2] = j;
                }
            }
            __syncthreads();
            const int enter = shi[2];
            if (enter < 0) {
                if (pass == 0) continue;
                if (shi[7]) status = kGuardSelect;               // a banned atom still asks to enter: reported, not hidden
                finished = true;
                break;
            }
            if (tid == 0) { inP[enter] = 1; plist[np] = enter; shi[0] = np + 1; }
            entered = enter;
            __syncthreads();
            break;
        }
        if (finished) break;
    }
    if (status != kSolved) {                                      // (the last iterate may be infeasible: a feasible one goes out, the counters report it)
        __syncthreads();
        for (int j = tid; j < n; j += nt) {
            if (inP[j]) { int r = 0; for (int k = 0; k < j; k++) r += inP[k]; plist[r] = j; }
        }
        if (tid == 0) { int c2 = 0; for (int k = 0; k < n; k++) c2 += inP[k]; shi[0] = c2; }
        __syncthreads();
        tile_residual(At, ldA, m, plist, shi[0], zat, true, yv, rv, tid);
    }
    *steps_out = steps_done;
    return status;
}

}  // namespace bpp
}  // namespace amx
