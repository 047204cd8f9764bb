// amx_batched_big.hip -- the batched nnls / lasso entry points on a dictionary marked DENSE (amx_dict_set_dense): supports of ANY size.
//
// The wavefront-per-voxel kernels of amx_batched.hip hold 16 passive atoms (main pass) and 48 (re-run pass); what does not fit there either is
// AMX_E_OVERFLOW on an ordinary dictionary.  On a dense one the re-run pass writes those voxels to a list of its own (launch_pair, big_after) and
// k_batched_big takes them from it, one WORKGROUP of 256 threads per voxel (the layout of k_noddi_lasso_big, amx_big.hip):
//     min_{x >= 0} 1/2 ||y - A x||^2 + lambda1 sum(x) + lambda2/2 ||x||^2              (nnls: lambda1 = lambda2 = 0)
// in Gram space, H = G_d + lambda2 I from the dictionary's Gram table (k_dict_gram, made once by amx_dict_set_dense), c = A_d'y - lambda1 from the
// fp64 tile where it lies.  Block principal pivoting from the kStart best single atoms: all infeasible atoms change sides while their number keeps
// falling (then kBackup more times), a dense Cholesky factorisation of H_PP per step -- packed, in LDS while the passive set fits (`lcap` atoms:
// what the 160 KB leave beside the vectors), in a global block per workgroup beyond.  Three things the NODDI kernel does not need:
//   1. thresholds relative to the problem (the signals are not normalised here): an inactive atom j is infeasible when its dual value exceeds
//      kTol sqrt(G_jj) ||y||, a passive one when z_j <= 0.  No absolute constant: x(c y) = c x(y), for lasso with lambda1 c.
//   2. a rank guard.  With lambda2 = 0, H_PP may be singular (a block step gathers more atoms than samples, or dependent ones): a pivot
//      <= kPiv H_jj drops that atom from P and the voxel goes on by SINGLE exchanges from x = 0.  Those are Lawson-Hanson's, not Murty's
//      least-index rule: Murty's is finite for a positive definite H only (restated in numpy, tests/batched_dense_np.py, every voxel of a 60 x 100
//      dictionary ran into the step cap with it).  The atom with the largest dual value per unit norm enters at the END of the pivot order -- so
//      only the entering atom can fail the pivot test --, atoms leave by the ratio test, the objective never rises.  A voxel whose block steps
//      stall takes the same road.  The step cap 4 n + 16 ends a voxel that does not settle: ST_ITCAP, never a hang.
//   3. a check on the TRUE problem before anything is written: r = y - A_P z and g = A'r - lambda2 z - lambda1 from the tile.  A passive |g_j|
//      above kTolP sqrt(G_jj) ||y|| asks for a refinement solve z += H_PP^-1 g_P (at most kRefine rounds, then ST_GUARD); an inactive atom with
//      a dual above its threshold, or a passive one the refinement turned non-positive, sends the voxel back into the pivoting.  rnorm = ||r||.
// The kernel takes its voxels from the device list and its device count alone (never perm[0 .. n): ADVICE.md).
#include "amx_launch.hpp"
using namespace amx;

namespace {

struct BigBatchedArgs {
    BatchedArgs a;
    const double *gram;           // [n_dicts][n][ldG]
    int ldG;
    const int *list;              // voxel numbers
    const int *count;             // their number (device)
    int lcap;                     // largest passive set whose packed factor lies in LDS
    double *Lg;                   // global factor blocks [gridDim.x][n (n + 1) / 2], or null (n <= lcap)
};

constexpr int kBbThreads = 256, kBbGrid = 256;
constexpr int kStart = 32, kBackup = 3, kRefine = 3;
constexpr double kTol = 1e-12, kTolP = 1e-11, kPiv = 1e-13;

__device__ __forceinline__ int tri_at(int r, int s) { return r * (r + 1) / 2 + s; }      // (<= 256 atoms: 32 896 entries)

// deterministic sum over the workgroup (the same tree whatever the data: the host and device forms agree bit for bit)
__device__ __forceinline__ double block_sum(double v, double *part, int tid)
{
    __syncthreads();
    part[tid] = v;
    __syncthreads();
    for (int w = kBbThreads / 2; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    const double t = part[0];
    __syncthreads();
    return t;
}

// out[j] = sum_i A[i][j] v[i], j < n: the threads over (row part, atom) so that a wavefront reads consecutive atoms of one row
__device__ __forceinline__ void tile_t_times(const double *__restrict__ At, int ldA, int m, int n, const double *v, double *out, double *part, int tid)
{
    const int parts = kBbThreads / n > 0 ? kBbThreads / n : 1;           // (n <= 256)
    __syncthreads();
    if (tid < parts * n) {
        const int j = tid % n, p = tid / n;
        double acc = 0.0;
        for (int i = p; i < m; i += parts) acc += At[(size_t)i * ldA + j] * v[i];
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
__device__ __forceinline__ void tile_residual(const double *__restrict__ At, int ldA, int m, const int *plist, int np, const double *x, bool clip,
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
                if (!clip || xj > 0.0) acc += At[(size_t)i * ldA + j] * xj;
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
__device__ __forceinline__ void factor_guarded(double *L, int np, const int *plist, const double *hd, int *drp, int *ndrop, double *col, int tid)
{
    __syncthreads();
    for (int k = 0; k < np; k++) {
        const double dk = L[tri_at(k, k)];
        const bool ok = dk > kPiv * hd[plist[k]];
        __syncthreads();                                     // (every thread has read the pivot)
        if (!ok) {
            for (int r = k + 1 + tid; r < np; r += kBbThreads) L[tri_at(r, k)] = 0.0;
            if (tid == 0) { drp[k] = 1; *ndrop += 1; }
            __syncthreads();
            continue;
        }
        const double d = sqrt(dk), di = 1.0 / d;
        for (int r = k + tid; r < np; r += kBbThreads) {
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
        for (int r = k + 1 + tid; r < np; r += kBbThreads) zv[r] -= L[tri_at(r, k)] * wk;
        __syncthreads();
    }
    for (int k = np - 1; k >= 0; k--) {
        const double zk = zv[k] / L[tri_at(k, k)];
        __syncthreads();
        if (tid == 0) zv[k] = zk;
        for (int r = tid; r < k; r += kBbThreads) zv[r] -= L[tri_at(k, r)] * zk;
        __syncthreads();
    }
}

// plist keeps the atoms still in P, in the order it holds them (tmp: n ints); *np_out = how many
__device__ __forceinline__ void compact_plist(int *plist, int np, const int *inP, int *tmp, int *np_out, int tid)
{
    __syncthreads();
    for (int r = tid; r < np; r += kBbThreads) {
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
    for (int r = tid; r < c2; r += kBbThreads) plist[r] = tmp[r];
    __syncthreads();
}

__global__ void __launch_bounds__(kBbThreads) k_batched_big(const BigBatchedArgs b)
{
    const BatchedArgs &a = b.a;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_bb[];
    const int m = a.c.nS, ldA = a.c.ldA, n = a.c.n_atoms;
    const int mp = (m + 1) & ~1, npd = (n + 1) & ~1, n4 = (n + 3) & ~3;
    double *yv = reinterpret_cast<double *>(smem_bb);              // [m] signal
    double *rv = yv + mp;                                          // [m] true residual
    double *cv = rv + mp;                                          // [n] c_j = a_j'y - lambda1
    double *zv = cv + npd;                                         // [n] right-hand side / solution in slot order
    double *zat = zv + npd;                                        // [n] solution in atom order
    double *xo = zat + npd;                                        // [n] the feasible point of the single exchanges
    double *gv = xo + npd;                                         // [n] dual values of the inactive atoms
    double *gtv = gv + npd;                                        // [n] gradient of the true problem
    double *thr = gtv + npd;                                       // [n] kTol sqrt(G_jj) ||y||
    double *hd = thr + npd;                                        // [n] H_jj
    double *sgd = hd + npd;                                        // [n] sqrt(G_jj)
    double *part = sgd + npd;                                      // [256] partial sums, scores, ratios
    double *dsc = part + kBbThreads;                               // [2] scalars
    int *plist = reinterpret_cast<int *>(dsc + 2);                 // [n] atoms of P in pivot order
    int *inP = plist + n4;                                         // [n] 1 = passive
    int *bad = inP + n4;                                           // [n] 1 = infeasible this step; scratch of compact_plist
    int *ban = bad + n4;                                           // [n] 1 = may not enter until x moves
    int *drp = ban + n4;                                           // [n] 1 = slot dropped by the rank guard
    int *shi = drp + n4;                                           // [16] scalars: 0 np, 1 n_bad, 2 entering atom, 3 dropped pivots, 4 non-finite, 5 passive z <= 0, 6 |g_P| above tolerance, 7 a banned atom asks to enter
    double *Ll = reinterpret_cast<double *>(shi + 16);             // packed lower triangle, <= lcap atoms
    double *Lg = b.Lg ? b.Lg + (size_t)blockIdx.x * ((size_t)n * (n + 1) / 2) : Ll;
    const int tid = threadIdx.x, nt = kBbThreads;
    const double *tiles = reinterpret_cast<const double *>(a.c.tiles);
    const double lam1 = a.c.lam1, lam2 = a.c.lam2;
    const int cnt = *b.count;

    for (int it = blockIdx.x; it < cnt; it += gridDim.x) {
        const int vox = b.list[it];
        const int dic = a.c.lutidx[vox];
        const double *At = tiles + (size_t)dic * a.c.tile_stride;
        const double *G = b.gram + (size_t)dic * n * b.ldG;
        double *dst = a.x + (size_t)vox * n;
        __syncthreads();
        if (tid < 16) shi[tid] = 0;
        __syncthreads();
        double yy = 0.0;
        for (int i = tid; i < m; i += nt) {
            const double yi = a.c.y[(size_t)vox * m + i];
            if (!(fabs(yi) <= 1.79769313486231570e308)) shi[4] = 1;
            yv[i] = yi; rv[i] = yi;
            yy += yi * yi;
        }
        const double ynorm = sqrt(block_sum(yy, part, tid));
        if (shi[4]) {                                             // non-finite signal: NaN out, like batched_voxel
            for (int j = tid; j < n; j += nt) dst[j] = __builtin_nan("");
            if (tid == 0 && a.rnorm) a.rnorm[vox] = __builtin_nan("");
            continue;
        }
        // ---- c, thresholds; the first passive set = the kStart atoms that fit the signal best on their own (c_j / sqrt(H_jj), c_j > 0)
        tile_t_times(At, ldA, m, n, yv, cv, part, tid);
        for (int j = tid; j < n; j += nt) {
            const double gjj = G[(size_t)j * b.ldG + j];
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
            for (int k = 0; k < n; k++) rank += (zat[k] > sj || (zat[k] == sj && k < j)) ? 1 : 0;
            inP[j] = (sj > 0.0 && rank < kStart) ? 1 : 0;
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
            const bool in_lds = np <= b.lcap;
            // ---- H_PP (packed lower triangle), the right-hand side
            for (int r = tid >> 4; r < np; r += 16) {
                const int pr = plist[r];
                const double *Gr = G + (size_t)pr * b.ldG;
                for (int s = tid & 15; s <= r; s += 16) {
                    const double h = Gr[plist[s]] + (s == r ? lam2 : 0.0);
                    if (in_lds) Ll[tri_at(r, s)] = h; else Lg[tri_at(r, s)] = h;
                }
            }
            for (int r = tid; r < np; r += nt) { zv[r] = cv[plist[r]]; drp[r] = 0; }
            if (in_lds) factor_guarded(Ll, np, plist, hd, drp, &shi[3], gtv, tid); else factor_guarded(Lg, np, plist, hd, drp, &shi[3], gtv, tid);      // (gtv is free until the true problem's pass)
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
                    const double *Gj = G + (size_t)j * b.ldG;
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
        // ---- out: the row of x (exact zeros off the support), ||r|| of the true residual
        if (status != kSolved) {                                      // (the last iterate may be infeasible: a feasible one goes out, the counters report it)
            __syncthreads();
            for (int j = tid; j < n; j += nt) {
                if (inP[j]) { int r = 0; for (int k = 0; k < j; k++) r += inP[k]; plist[r] = j; }
            }
            if (tid == 0) { int c2 = 0; for (int k = 0; k < n; k++) c2 += inP[k]; shi[0] = c2; }
            __syncthreads();
            tile_residual(At, ldA, m, plist, shi[0], zat, true, yv, rv, tid);
        }
        if (status == kIterCap && tid == 0) atomicAdd(&a.c.status[ST_ITCAP], 1);
        if (status > kIterCap && tid == 0) { atomicAdd(&a.c.status[ST_GUARD], 1); a.c.status[ST_GUARDVOX] = vox * 8 + status; }
        for (int j = tid; j < n; j += nt) dst[j] = (inP[j] && zat[j] > 0.0) ? zat[j] : 0.0;
        if (a.rnorm) {
            double rr = 0.0;
            for (int i = tid; i < m; i += nt) rr += rv[i] * rv[i];
            rr = block_sum(rr, part, tid);
            if (tid == 0) a.rnorm[vox] = sqrt(rr);
        }
        if (tid == 0) { atomicAdd(&a.c.status[ST_DENSE], 1); atomicAdd(&a.c.status[ST_DENSE + 1], steps_done); }
    }
}

size_t bb_vec_bytes(int m, int n)
{
    const size_t mp = (size_t)((m + 1) & ~1), npd = (size_t)((n + 1) & ~1), n4 = (size_t)((n + 3) & ~3);
    size_t bytes = (2 * mp + 9 * npd + kBbThreads + 2) * sizeof(double) + (5 * n4 + 16) * sizeof(int);
    return (bytes + 15) & ~(size_t)15;
}

// G_d = A_d'A_d, one workgroup per (dictionary, row): the row's atom is read by every thread, the other atom across the threads
__global__ void __launch_bounds__(256) k_dict_gram(const double *__restrict__ tiles, int m, int n, int ldA, int tile_stride, int ldG, double *__restrict__ G)
{
    const int d = blockIdx.x / n, j = blockIdx.x % n, k = threadIdx.x;
    if (k >= ldG) return;
    const double *At = tiles + (size_t)d * tile_stride;
    double acc = 0.0;
    if (k < n)
        for (int i = 0; i < m; i++) acc += At[(size_t)i * ldA + j] * At[(size_t)i * ldA + k];
    G[((size_t)d * n + j) * ldG + k] = acc;
}

}  // namespace

// the voxels the 48-atom re-run pass of a dense dictionary wrote to list 6 (launch_pair, big_after): one launch, whatever their number
int amx_launch_batched_big(amx_ctx *ctx, const BatchedArgs &a, const amx_dict *dict, const Plan &pl, hipStream_t s)
{
    BigBatchedArgs b;
    memset(&b, 0, sizeof b);
    b.a = a; b.gram = dict->gram; b.ldG = dict->ldG;
    b.list = pl.ovf_list + (size_t)6 * pl.n; b.count = pl.ovf_count + 10;
    const int m = a.c.nS, n = a.c.n_atoms;
    const size_t vec = bb_vec_bytes(m, n);
    if (vec > kLdsPerCU) { ctx->err = "k_batched_big: the dictionary's vectors do not fit the LDS"; return AMX_E_BADARG; }
    int lcap = 0;
    while (lcap < n && vec + ((size_t)(lcap + 1) * (lcap + 2) / 2) * sizeof(double) <= kLdsPerCU) lcap++;
    b.lcap = lcap;
    int rc;
    if (lcap < n) {
        if ((rc = amx_ensure(ctx, ctx->big, (size_t)kBbGrid * ((size_t)n * (n + 1) / 2) * sizeof(double)))) return rc;
        b.Lg = (double *)ctx->big.p;
    }
    const size_t lds = vec + ((size_t)lcap * (lcap + 1) / 2) * sizeof(double);
    rec(ctx, 4, s);
    if ((rc = launch_lds(ctx, k_batched_big, dim3(kBbGrid), dim3(kBbThreads), lds, s, b))) return rc;
    amx_note(ctx, "k_batched_big (dense dictionary: supports beyond 48 atoms)");
    AMX_TRACE(ctx, s, "batched solvers, any support size (block principal pivoting, workgroup per voxel)");
    rec(ctx, 5, s);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

// G_d of every dictionary of `dict` into dict->gram (allocated by the caller: amx_dict_set_dense), on the null stream
int amx_build_dict_gram(amx_ctx *ctx, const amx_dict *dict)
{
    hipLaunchKernelGGL(k_dict_gram, dim3((unsigned)((size_t)dict->n_dicts * dict->n)), dim3(256), 0, nullptr, dict->tiles, dict->m, dict->n, dict->ldA,
                       dict->tile_stride, dict->ldG, dict->gram);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}
