// amx_sandi_lane.hip -- SANDI, one voxel per lane (amx_lane_qp.hpp): k_sandi_lane, and the row-space solver of the default
// protocol (k_sandi_tables, k_sandi_rows)
#include "amx_lane_qp.hpp"

namespace {

template <int N>
__global__ void __launch_bounds__(256) k_sandi_lane(const SandiArgs a)
{
    AMX_SMALL_LDS(double)
    const int cid = xcd_chunk((int)blockIdx.x, *a.c.n_chunks);
    if (cid < 0) return;
    const Chunk ck = a.c.chunks[cid];
    const int nS = a.c.nS, ldA = a.c.ldA, n_atoms = a.c.n_atoms, n_rs = a.n_rs, n_in = a.n_in;
    small_prologue<N, double>(reinterpret_cast<const double *>(a.c.tiles), words, As, Hs, nS, ldA, n_atoms, a.c.lam2);
    for (int v = threadIdx.x; v < ck.count; v += blockDim.x) {
        const int vox = a.c.perm[ck.start + v];
        const double *yv = a.c.y + (size_t)vox * nS;
        double c[N], x[N], ysq;
        const bool ok = lane_aty<N, double>(As, yv, nS, ldA, n_atoms, c, ysq);
        double *e = a.est + (size_t)vox * 6;
        if (!ok) {
            const double nan = __builtin_nan("");
            for (int m = 0; m < 6; m++) e[m] = nan;
            if (a.rmse) a.rmse[vox] = nan;
            if (a.nrmse) a.nrmse[vox] = nan;
            continue;
        }
#pragma unroll
        for (int j = 0; j < N; j++) c[j] -= a.c.lam1;
        if (lane_nnqp<N>(Hs, c, x, n_atoms, amx_warm_start(a.c.lam2, a.c.flags)) != 0) atomicAdd(&a.c.status[ST_ITCAP], 1);
        // models.pyx:1570-1612
        double x_sum = 0.0, xsph = 0.0, xstk = 0.0, xiso = 0.0, Rsoma = 0.0, Din = 0.0, De = 0.0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            if (j < n_atoms) {
                x[j] *= a.norms[j];
                x_sum += x[j];
                if (j < n_rs) { xsph += x[j]; Rsoma += a.Rs[j] * x[j]; }
                else if (j < n_rs + n_in) { xstk += x[j]; Din += a.d_in[j - n_rs] * x[j]; }
                else { xiso += x[j]; De += a.d_isos[j - n_rs - n_in] * x[j]; }
            }
        }
        if (a.c.xdbg) {                                   // the rescaled x (models.pyx:1570-1571)
#pragma unroll
            for (int j = 0; j < N; j++) if (j < n_atoms) a.c.xdbg[(size_t)vox * n_atoms + j] = x[j];
        }
        x_sum += 1e-16;
        e[0] = fast_div(xsph, x_sum); e[1] = fast_div(xstk, x_sum); e[2] = fast_div(xiso, x_sum);
        e[3] = 1e6 * fast_div(Rsoma, xsph + 1e-16);
        e[4] = 1e3 * fast_div(Din, xstk + 1e-16);
        e[5] = 1e3 * fast_div(De, xiso + 1e-16);
        if (a.rmse || a.nrmse) {
            // quirk kept (models.pyx:1571 then 1615): errors use the RESCALED x with the NORMALISED A
            const double rss = lane_rss<N, double>(As, yv, nS, ldA, n_atoms, x);
            if (a.rmse) a.rmse[vox] = sqrt(rss / (double)nS);
            if (a.nrmse) a.nrmse[vox] = (ysq > 1e-16) ? sqrt(rss / ysq) : 0.0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Row-space solver of the SANDI problem (M = 6 values per voxel after the directional average, N = 15 atoms, ONE dictionary
// for all voxels):  min 1/2 ||y - A x||^2 + lambda1 sum(x) + lambda2/2 ||x||^2, x >= 0, lambda2 > 0.
// On a passive set P the solution is x_P = (c_P - A_P' w) / lambda2 with w = B^-1 A_P c_P, B = lambda2 I + A_P A_P' (Woodbury:
// a 6 x 6 Cholesky instead of a |P| x |P| one).  For j outside P the same expression is the dual value: A_P x_P = w exactly,
// so g_j = c_j - a_j'w -- the KKT test and the choice of the entering atom cost nothing extra.
// Tables of the dictionary (k_sandi_tables, once per (dictionary, lambda1, lambda2)), read with wave-uniform addresses (scalar loads):
//   T [N][kRowsTs]  packed lower triangles of a_j a_j'          (B is summed from them: no +- drift, half the arithmetic)
//   G [N][M], g0 [N]  z0 = G y + g0 = the unconstrained optimum on the FULL set (G = A' (lambda2 I + A A')^-1)
// Warm start: SANDI's optimum is dense (12 of 15 atoms), so the method starts from P0 = {z0 > 0} -- the full-set solve and
// the first block removal are one tabulated map -- and continues by block principal pivoting (below).  With lambda2 > 0
// the optimum is unique, so the path does not matter; the result satisfies the KKT conditions to 1e-12.
constexpr int kRowsTs = 22;                // stride of T: 21 entries of the 6 x 6 triangle, padded for 16-byte reads

template <int M, int N, typename TP>
__device__ __forceinline__ int lane_nnqp_rows(TP A, int ldA, TP T, TP G, TP g0, const double (&y)[M],
                                              double lam1, double lam2, double (&x)[N], int n_atoms, bool warm)
{
    static_assert(M * (M + 1) / 2 <= kRowsTs, "triangle of a_j a_j' fits its table row");
    constexpr int kTri = M * (M + 1) / 2;
    const double il2 = 1.0 / lam2;
    // the dual test follows the voxel's own scale (lane_nnqp): the atoms are normalised, so |c_j| <= ||y|| -- max |y| stands for it
    double ymax = 0.0;
#pragma unroll
    for (int i = 0; i < M; i++) ymax = fmax(ymax, fabs(y[i]));
    const double tol = 1e-12 * fmin(ymax, 1.0);
    // c = A'y - lambda1 is never stored (15 doubles = 30 registers the Cholesky would have to live with): c_j is recomputed for
    // the atoms that change sides (below), the dual values are g_j = a_j'(y - w) - lambda1.
    unsigned P = 0u;
    AMX_RELOAD();
#pragma unroll
    for (int j = 0; j < N; j++) {
        x[j] = 0.0;
        double sz = g0[j];
#pragma unroll
        for (int i = 0; i < M; i++) sz += G[j * M + i] * y[i];
        if (warm && j < n_atoms && sz > 0.0) P |= 1u << j;
    }
    constexpr int kBackup = 3;               // block exchanges allowed without progress (Kim & Park)
    int ninf = N + 1, backup = 0;
    // A_P A_P' and the right-hand side A_P c_P are CARRIED from trip to trip: only the atoms that changed sides are added or
    // subtracted (rank-one terms from the table, a_j c_j with c_j = a_j'y - lambda1 recomputed on the spot).  The branch per atom
    // is wave-uniform (ballot over the lanes still iterating): in the late trips of a lock-step wavefront few lanes are left and
    // they exchange one or two atoms each.  (+- accumulation: a handful of updates per voxel, errors of 1e-16 relative.)
    double Bp[kTri], rp[M];
#pragma unroll
    for (int t = 0; t < kTri; t++) Bp[t] = 0.0;
#pragma unroll
    for (int i = 0; i < M; i++) rp[i] = 0.0;
    unsigned flips = P;
    for (int it = 0;; ++it) {
        if (it > 4 * N + 16) return 2;
        double B[kTri], L[kTri], li[M], w[M];
        AMX_RELOAD();
#pragma unroll
        for (int j = 0; j < N; j++) {
            const bool fj = (flips >> j) & 1u;
            if (__ballot(fj) != 0ull) {
                const double dj = fj ? (((P >> j) & 1u) ? 1.0 : -1.0) : 0.0;
                double cj = -lam1;
#pragma unroll
                for (int i = 0; i < M; i++) cj += A[i * ldA + j] * y[i];
                cj *= dj;
#pragma unroll
                for (int t = 0; t < kTri; t++) Bp[t] += dj * T[j * kRowsTs + t];
#pragma unroll
                for (int i = 0; i < M; i++) rp[i] += cj * A[i * ldA + j];
            }
        }
#pragma unroll
        for (int t = 0; t < kTri; t++) B[t] = Bp[t];
#pragma unroll
        for (int i = 0; i < M; i++) { w[i] = rp[i]; B[tri<M>(i, i)] += lam2; }
#pragma unroll
        for (int j = 0; j < M; j++) {
            double d = B[tri<M>(j, j)];
#pragma unroll
            for (int k = 0; k < j; k++) d -= L[tri<M>(j, k)] * L[tri<M>(j, k)];
            const double iv = rsqrt(d);
            li[j] = iv;
#pragma unroll
            for (int i = j + 1; i < M; i++) {
                double tt = B[tri<M>(i, j)];
#pragma unroll
                for (int k = 0; k < j; k++) tt -= L[tri<M>(i, k)] * L[tri<M>(j, k)];
                L[tri<M>(i, j)] = tt * iv;
            }
        }
#pragma unroll
        for (int j = 0; j < M; j++) {
            double sacc = w[j];
#pragma unroll
            for (int k = 0; k < j; k++) sacc -= L[tri<M>(j, k)] * w[k];
            w[j] = sacc * li[j];
        }
#pragma unroll
        for (int j = M - 1; j >= 0; j--) {
            double sacc = w[j];
#pragma unroll
            for (int i = j + 1; i < M; i++) sacc -= L[tri<M>(i, j)] * w[i];
            w[j] = sacc * li[j];
        }
        AMX_RELOAD();
        // block principal pivoting: passive atoms with a non-positive coefficient leave, inactive atoms with a positive dual
        // value enter, all at once while the number of infeasibilities keeps falling (then kBackup more times); otherwise only
        // the infeasible atom with the largest index is exchanged (Murty's rule).  (Launched with the warm start only: smaller
        // lambda2 / flag bit 31 (cold start) go to k_sandi_lane's Lawson-Hanson loop, amx_launch_sandi_small.)
        unsigned v1 = 0u, v2 = 0u;
#pragma unroll
        for (int i = 0; i < M; i++) w[i] = y[i] - w[i];
#pragma unroll
        for (int j = 0; j < N; j++) {
            double g = -lam1;
#pragma unroll
            for (int i = 0; i < M; i++) g += A[i * ldA + j] * w[i];
            const bool pj = (P >> j) & 1u;
            x[j] = pj ? g * il2 : 0.0;
            if (pj && !(g > 0.0)) v1 |= 1u << j;
            if (!pj && j < n_atoms && g > tol) v2 |= 1u << j;
        }
        const unsigned bad = v1 | v2;
        if (bad == 0u) return 0;                                   // KKT point: x holds the solution
        const int nbad = __builtin_popcount(bad);
        bool block = false;
        if (nbad < ninf) { ninf = nbad; backup = warm ? kBackup : 0; block = warm; }
        else if (backup > 0) { backup--; block = true; }
        flips = block ? bad : (1u << (31 - __builtin_clz(bad)));
        P ^= flips;
    }
}

// T, G, g0 of one dictionary and one (lambda1, lambda2): one workgroup, thread 0 inverts the 6 x 6 (Gauss-Jordan on the SPD
// matrix, no pivoting needed).  out: T [N][kRowsTs] | G [N][M] | g0 [16] | A [M][16] (zero-padded rows)
template <int M, int N>
__global__ void __launch_bounds__(64) k_sandi_tables(const double *__restrict__ Ag, int ldA, int n_atoms, double lam1, double lam2,
                                                     double *__restrict__ out)
{
    __shared__ double A[M * 16], W[M * M], Bm[M * 2 * M];
    for (int e = threadIdx.x; e < M * 16; e += blockDim.x) A[e] = ((e % 16) < n_atoms) ? Ag[(e / 16) * ldA + (e % 16)] : 0.0;
    __syncthreads();
    double *T = out, *G = out + N * kRowsTs, *g0 = G + N * M;
    for (int e = threadIdx.x; e < M * 16; e += blockDim.x) g0[16 + e] = A[e];                // the dictionary, rows padded to 16
    for (int e = threadIdx.x; e < N * kRowsTs; e += blockDim.x) {
        const int j = e / kRowsTs, t = e % kRowsTs;
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= t) i++;                 // t = i (i + 1) / 2 + k
        const int k = t - i * (i + 1) / 2;
        T[e] = (t < M * (M + 1) / 2) ? A[i * 16 + j] * A[k * 16 + j] : 0.0;
    }
    if (threadIdx.x == 0) {
        for (int i = 0; i < M; i++)
            for (int k = 0; k < M; k++) {
                double acc = (i == k) ? lam2 : 0.0;
                for (int j = 0; j < N; j++) acc += A[i * 16 + j] * A[k * 16 + j];
                Bm[i * 2 * M + k] = acc; Bm[i * 2 * M + M + k] = (i == k) ? 1.0 : 0.0;
            }
        for (int c0 = 0; c0 < M; c0++) {
            const double pv = 1.0 / Bm[c0 * 2 * M + c0];
            for (int k = 0; k < 2 * M; k++) Bm[c0 * 2 * M + k] *= pv;
            for (int i = 0; i < M; i++)
                if (i != c0) {
                    const double f = Bm[i * 2 * M + c0];
                    for (int k = 0; k < 2 * M; k++) Bm[i * 2 * M + k] -= f * Bm[c0 * 2 * M + k];
                }
        }
        for (int i = 0; i < M; i++) for (int k = 0; k < M; k++) W[i * M + k] = Bm[i * 2 * M + M + k];
    }
    __syncthreads();
    // z0 = (c - A' W A c) / lambda2 with c = A'y - lambda1 1 and A A' = W^-1 - lambda2 I:
    //    = A' W y - (lambda1 / lambda2) (1 - A' W A 1)
    for (int e = threadIdx.x; e < N * M; e += blockDim.x) {
        const int j = e / M, i = e % M;
        double acc = 0.0;
        for (int k = 0; k < M; k++) acc += A[k * 16 + j] * W[k * M + i];
        G[e] = acc;
    }
    for (int j = threadIdx.x; j < 16; j += blockDim.x) {
        double acc = 0.0;
        if (j < n_atoms) {
            double awa = 0.0;
            for (int i = 0; i < M; i++) {
                double wi = 0.0;
                for (int k = 0; k < M; k++) { double a1 = 0.0; for (int jj = 0; jj < n_atoms; jj++) a1 += A[k * 16 + jj]; wi += W[i * M + k] * a1; }
                awa += A[i * 16 + j] * wi;
            }
            acc = -(lam1 / lam2) * (1.0 - awa);
        }
        g0[j] = acc;
    }
}
constexpr int kSandiTableWords = 15 * kRowsTs + 15 * 6 + 16 + 8 * 16;

constexpr int kRowsOcc = 3;

// SANDI, nS == M (<= 8) values per voxel: row-space solver; the dictionary and its tables come through the scalar cache
// (wave-uniform addresses), y from the voxel's row.
template <int M, int N>
__global__ void __launch_bounds__(256, kRowsOcc) k_sandi_rows(const SandiArgs a)
{
    Chunk ck;
    const bool linear = a.n_lin > 0;           // SANDI has one dictionary: nothing to bucket, the voxels are taken in order
    if (linear) {
        ck.start = (int)blockIdx.x * 256; ck.count = a.n_lin - ck.start < 256 ? a.n_lin - ck.start : 256;
        if (ck.count <= 0) return;
    } else {
        const int cid = xcd_chunk((int)blockIdx.x, *a.c.n_chunks);
        if (cid < 0) return;
        ck = a.c.chunks[cid];
    }
    const int n_atoms = a.c.n_atoms, n_rs = a.n_rs, n_in = a.n_in;
    // the dictionary and its tables (4.6 KB, the same for every voxel) are read through the SCALAR cache: every address is
    // wave-uniform, so the loads are s_load_dwordx8/x16 into SGPRs and the fused multiply-adds take them as their scalar
    // operand -- no LDS instruction in the solver (from LDS the ~210 16-byte broadcast reads per trip cost as much of the
    // CU's time as the ~650 fp64 instructions they feed).
    using CD = const __attribute__((address_space(4))) double;
    constexpr int ldA = 16;
    CD *T = (CD *)a.tables, *G = T + N * kRowsTs, *g0 = G + N * M, *A = g0 + 16;
    const bool warm = amx_warm_start(a.c.lam2, a.c.flags);
    // the atoms' norms and model parameters (Rs | d_in | d_isos by atom class) once per workgroup: read in the maps section below
    // from their four arrays, every value was a load of its own under a wave-uniform guard, waited for before the next one left --
    // ~45 memory round trips one after the other per wavefront, as long as the solver itself
    __shared__ double s_par[2][16];
    if (threadIdx.x < 16) {
        const int j = threadIdx.x;
        s_par[0][j] = j < n_atoms ? a.norms[j] : 0.0;
        s_par[1][j] = j < n_rs ? a.Rs[j] : (j < n_rs + n_in ? a.d_in[j - n_rs] : (j < n_atoms ? a.d_isos[j - n_rs - n_in] : 0.0));
    }
    __syncthreads();
    for (int v = threadIdx.x; v < ck.count; v += blockDim.x) {
        const int vox = linear ? ck.start + v : a.c.perm[ck.start + v];
        const double *yv = a.c.y + (size_t)vox * M;
        double y[M], x[N], ysq = 0.0;
        bool ok = true;
#pragma unroll
        for (int i = 0; i < M; i++) {
            y[i] = yv[i];
            ok = ok && (fabs(y[i]) <= 1.79769313486231570e308);
            ysq += y[i] * y[i];
        }
        double *e = a.est + (size_t)vox * 6;
        if (!ok) {
            const double nan = __builtin_nan("");
            for (int m = 0; m < 6; m++) e[m] = nan;
            if (a.rmse) a.rmse[vox] = nan;
            if (a.nrmse) a.nrmse[vox] = nan;
            continue;
        }
        if (lane_nnqp_rows<M, N>(A, ldA, T, G, g0, y, a.c.lam1, a.c.lam2, x, n_atoms, warm) != 0) atomicAdd(&a.c.status[ST_ITCAP], 1);
        // models.pyx:1570-1612
        double x_sum = 0.0, xsph = 0.0, xstk = 0.0, xiso = 0.0, Rsoma = 0.0, Din = 0.0, De = 0.0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const double nj = s_par[0][j < 16 ? j : 0], pj = s_par[1][j < 16 ? j : 0];
            if (j < n_atoms) {
                x[j] *= nj;
                x_sum += x[j];
                if (j < n_rs) { xsph += x[j]; Rsoma += pj * x[j]; }
                else if (j < n_rs + n_in) { xstk += x[j]; Din += pj * x[j]; }
                else { xiso += x[j]; De += pj * x[j]; }
            }
        }
        if (a.c.xdbg) {                                   // the rescaled x (models.pyx:1570-1571)
#pragma unroll
            for (int j = 0; j < N; j++) if (j < n_atoms) a.c.xdbg[(size_t)vox * n_atoms + j] = x[j];
        }
        x_sum += 1e-16;
        e[0] = fast_div(xsph, x_sum); e[1] = fast_div(xstk, x_sum); e[2] = fast_div(xiso, x_sum);
        e[3] = 1e6 * fast_div(Rsoma, xsph + 1e-16);
        e[4] = 1e3 * fast_div(Din, xstk + 1e-16);
        e[5] = 1e3 * fast_div(De, xiso + 1e-16);
        if (a.rmse || a.nrmse) {
            // quirk kept (models.pyx:1571 then 1615): errors use the RESCALED x with the NORMALISED A
            double rss = 0.0;
#pragma unroll
            for (int i = 0; i < M; i++) {
                double ei = y[i];
#pragma unroll
                for (int j = 0; j < N; j++) ei -= A[i * ldA + j] * x[j];
                rss += ei * ei;
            }
            if (a.rmse) a.rmse[vox] = sqrt(rss / (double)M);
            if (a.nrmse) a.nrmse[vox] = (ysq > 1e-16) ? sqrt(rss / ysq) : 0.0;
        }
    }
}

}  // namespace

size_t amx_sandi_table_words() { return (size_t)kSandiTableWords; }      // (amx_debug_fetch)

// tables of the row-space solver, cached in the dictionary handle for one (lambda1, lambda2)
int amx_sandi_prepare(amx_ctx *ctx, const amx_lut *lut, SandiArgs &a, hipStream_t s)
{
    if (lut->sandi_lam1 != a.c.lam1 || lut->sandi_lam2 != a.c.lam2 || !lut->sandi_prep) {
        if (lut->sandi_prep) HIPCHK(ctx, hipDeviceSynchronize());                              // (a fit with the old tables may still run)
        if (!lut->sandi_prep) HIPCHK(ctx, hipMalloc((void **)&lut->sandi_prep, kSandiTableWords * sizeof(double)));
        if (!lut->sandi_ready) HIPCHK(ctx, hipEventCreateWithFlags(&lut->sandi_ready, hipEventDisableTiming));
        hipLaunchKernelGGL((k_sandi_tables<6, 15>), dim3(1), dim3(64), 0, s, reinterpret_cast<const double *>(lut->tiles), lut->ldA,
                           lut->n_atoms, a.c.lam1, a.c.lam2, lut->sandi_prep);
        AMX_TRACE(ctx, s, "SANDI dictionary tables");
        HIPCHK(ctx, hipEventRecord(lut->sandi_ready, s));
        lut->sandi_lam1 = a.c.lam1; lut->sandi_lam2 = a.c.lam2;
    }
    HIPCHK(ctx, hipStreamWaitEvent(s, lut->sandi_ready, 0));
    a.tables = lut->sandi_prep;
    return AMX_OK;
}

int amx_launch_sandi_small(amx_ctx *ctx, SandiArgs &a, const Plan &pl, hipStream_t s, const SmallRoute &rt)
{
    // the default protocol after the directional average (b0 + 5 shells = 6 values, 15 atoms: SANDI's default 5 + 5 + 5): row-space solver
    // (a refill variant of this kernel -- lanes drawing the next voxel from a global counter -- was measured SLOWER,
    //  2.65 vs 2.29 ms per 1 M voxels: SANDI's optimum is dense, 12 of 15 atoms, so the lanes of a wavefront need
    //  nearly the same number of steps and there is no idle time to win back)
    if (rt.family == SF_SANDI_ROWS) {
        rec(ctx, 2, s);
        hipLaunchKernelGGL((k_sandi_rows<6, 15>), dim3(a.n_lin > 0 ? (a.n_lin + 255) / 256 : ((pl.max_chunks + 7) / 8) * 8), dim3(256), 0, s, a);
        amx_note(ctx, rt.launch[0]);
        AMX_TRACE(ctx, s, "row-space SANDI solver");
        rec(ctx, 3, s);
        HIPCHK(ctx, hipGetLastError());
        return AMX_OK;
    }
    if (rt.N == 12) return launch_lane(ctx, a, pl, s, k_sandi_lane<12>, rt);
    if (rt.N == 15) return launch_lane(ctx, a, pl, s, k_sandi_lane<15>, rt);
    return launch_lane(ctx, a, pl, s, k_sandi_lane<16>, rt);
}
