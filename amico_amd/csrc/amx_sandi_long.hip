// amx_sandi_long.hip -- SANDI on protocols of 129 .. 512 volumes (no directional average; models.pyx:1567-1619).
//
// SANDI has ONE dictionary for all voxels, and with lambda2 > 0 all a voxel contributes to its problem
//     min_x 1/2 ||y - A x||^2 + lambda1 sum(x) + lambda2/2 ||x||^2,  x >= 0
// is c = A'y (n_atoms numbers) and y'y: one GEMM over the signals, the only pass over y, then a Gram-space problem on
// H = A'A + lambda2 I per voxel.  (The kernels of the short protocols hold the signal rows in a lane's registers, or let every lane walk
// its own row: at 306 volumes the first spills and the second touches 64 cache lines per load.)
//   k_sandi_long_tables  once per (dictionary, lambda2): G = A'A, H = G + lambda2 I (identity on the padding atoms), both padded to whole
//                        16-atom tiles, and A' in MFMA operand order
//   k_sandi_project      c = A'y (raw: before - lambda1), y'y and a finite flag of every voxel on the fp64 matrix cores; float64 or float32
//                        signals, read in place; handed over in atom-major blocks of 64 voxels
//   k_sandi_gram_lane<N> n_atoms <= 16: one voxel per lane, H in LDS, lane_nnqp<N> (amx_lane_qp.hpp), the maps
//   k_sandi_gram_wave    n_atoms <= 64 (or AMX_WAVE_PER_VOXEL=1): one wavefront per voxel, lane = atom, block principal pivoting with
//                        Murty's fallback on a packed Cholesky factor in LDS (the loop of k_noddi_lasso_big, amx_big.hip)
// The error maps come from the Gram identity rss = y'y - 2 x'c + x'G x with the RESCALED x (the reference's quirk, models.pyx:1571 then
// 1615, as k_sandi_lane keeps it): no second pass over y.  The quirk leaves rmse ~ 0.4 on unit signals, so nothing cancels.
// Without a ridge (lambda2 < 1e-9) the route does not exist: an isotropic dictionary has rank <= shells + 1 < n_atoms, G alone is singular.
#include "amx_lane_qp.hpp"

namespace {

struct SandiLongArgs {
    const double *y; const float *y32;       // [n][nS], one of the two
    int n, nS, n_atoms, n_rs, n_in;
    int NP;                                  // atoms, padded to whole 16-atom tiles
    int ksteps;                              // K steps of the projection: 4 per 16 volumes, the last chunk zero-padded
    int rows;                                // rows of a hand-over block: NP atoms, y'y, the finite flag
    const double *G, *H, *At;                // k_sandi_long_tables: [NP][NP], [NP][NP], [NP / 16][ksteps][64]
    const double *norms, *Rs, *d_in, *d_isos;
    double lam1, lam2;
    unsigned flags;
    double *Cb;                              // [n_blocks][rows][64]: the hand-over, atom-major blocks of 64 voxels
    double *est, *rmse, *nrmse, *xdbg;
    int *status;
};

// K order of the projection: step s of lane quarter q takes volume 16 (s / 4) + 4 q + (s % 4) -- the sum over K may run in any order
// as long as both operands agree on it, and in this one a lane's four consecutive steps read four CONSECUTIVE samples of its voxel (one
// 16- or 32-byte load; the four quarters together 64 or 128 contiguous bytes of the row) instead of one sample every 4.
__host__ __device__ constexpr int sl_volume(int s, int q) { return 16 * (s >> 2) + 4 * q + (s & 3); }

__global__ void __launch_bounds__(256) k_sandi_long_tables(const double *__restrict__ A, int nS, int ldA, int n_atoms, double lam2, int NP,
                                                           int ksteps, double *__restrict__ out)
{
    double *G = out, *H = out + NP * NP, *At = H + NP * NP;
    const int t0 = (int)(blockIdx.x * blockDim.x + threadIdx.x), nt = (int)(gridDim.x * blockDim.x);
    for (int e = t0; e < NP * NP; e += nt) {
        const int j = e / NP, k = e - j * NP;
        double acc = 0.0;
        if (j < n_atoms && k < n_atoms)
            for (int i = 0; i < nS; i++) acc += A[(size_t)i * ldA + j] * A[(size_t)i * ldA + k];
        G[e] = acc;
        H[e] = acc + (j == k ? (j < n_atoms ? lam2 : 1.0) : 0.0);
    }
    for (int e = t0; e < (NP >> 4) * ksteps * 64; e += nt) {
        const int l = e & 63, s = (e >> 6) % ksteps, mt = (e >> 6) / ksteps;
        const int atom = 16 * mt + (l & 15), i = sl_volume(s, l >> 4);
        At[e] = (i < nS && atom < n_atoms) ? A[(size_t)i * ldA + atom] : 0.0;
    }
}

// One workgroup = 4 wavefronts; a wavefront takes 16 voxels of a 64-voxel block at a time (the N side of the 16 x 16 x 4 MFMA), the M side
// is one tile of 16 atoms, whose operand (ksteps x 64 doubles: 64 KB at 512 volumes) sits in LDS.  Dictionaries of more than 16 atoms take
// one pass over the signals per atom tile.
template <typename T>
__global__ void __launch_bounds__(256) k_sandi_project(const SandiLongArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_p[];
    double *As = reinterpret_cast<double *>(smem_p);
    const T *yg = reinterpret_cast<const T *>(sizeof(T) == 4 ? (const void *)a.y32 : (const void *)a.y);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, c16 = lane & 15, nS = a.nS, KS = a.ksteps, NT = a.NP >> 4;
    const int n_blk = (a.n + 63) >> 6;
    const int n_full = nS >> 4;                  // chunks of 16 volumes that every lane quarter reads whole
    constexpr int CB = 4;                        // chunks in flight: 4 loads of 4 samples per lane
    typedef double v4d __attribute__((ext_vector_type(4)));
    for (int mt = 0; mt < NT; mt++) {
        __syncthreads();
        const double *Ag = a.At + (size_t)mt * KS * 64;
        for (int e = threadIdx.x; e < KS * 64; e += (int)blockDim.x) As[e] = Ag[e];
        __syncthreads();
        for (int bl = blockIdx.x; bl < n_blk; bl += (int)gridDim.x) {
            if (64 * bl + 16 * wave >= a.n) continue;                       // (wave-uniform: the whole group lies past the end)
            const int v = 64 * bl + 16 * wave + c16;
            const bool live = v < a.n;
            // rows are aligned to their element only (129 float32 values: 516 bytes): the 4-sample loads are element-aligned copies
            const T *yv = yg + (size_t)(live ? v : a.n - 1) * nS + 4 * q;
            v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
            double ysq = 0.0;
            bool fin = true;
            for (int c0 = 0; c0 < n_full; c0 += CB) {
                T yb[CB][4];
#pragma unroll
                for (int u = 0; u < CB; u++) {
                    const int c = c0 + u < n_full ? c0 + u : n_full - 1;
                    __builtin_memcpy(yb[u], yv + 16 * c, 4 * sizeof(T));
                }
#pragma unroll
                for (int u = 0; u < CB; u++) {
                    if (c0 + u < n_full) {
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const double b = live ? (double)yb[u][j] : 0.0;
                            fin = fin && (fabs(b) <= 1.79769313486231570e308);      // per sample: (1e200)^2 overflows the sum
                            ysq += b * b;
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(4 * (c0 + u) + j) * 64 + lane], b, acc, 0, 0, 0);
                        }
                    }
                }
            }
            if (4 * n_full < KS) {                                          // the K tail: guarded loads, zeros beyond the row
                T yt[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int i = 16 * n_full + 4 * q + j;
                    yt[j] = yv[16 * n_full + (i < nS ? j : -4 * q - 16 * n_full)];      // (beyond the row: the row's first sample, discarded)
                    yt[j] = i < nS ? yt[j] : (T)0;
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double b = live ? (double)yt[j] : 0.0;
                    fin = fin && (fabs(b) <= 1.79769313486231570e308);
                    ysq += b * b;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(4 * n_full + j) * 64 + lane], b, acc, 0, 0, 0);
                }
            }
            double *out = a.Cb + (size_t)bl * a.rows * 64 + 16 * wave + c16;
            if (live) {
#pragma unroll
                for (int rr = 0; rr < 4; rr++) out[(size_t)(16 * mt + 4 * rr + q) * 64] = acc[rr];      // C/D of the f64 MFMA: row = quarter + 4 reg
            }
            if (mt == 0) {
                ysq += __shfl_xor(ysq, 16);
                ysq += __shfl_xor(ysq, 32);
                int f = fin ? 1 : 0;
                f &= __shfl_xor(f, 16);
                f &= __shfl_xor(f, 32);
                if (live && q == 0) { out[(size_t)a.NP * 64] = ysq; out[(size_t)(a.NP + 1) * 64] = f ? 1.0 : 0.0; }
            }
        }
    }
}

__device__ __forceinline__ void sl_nan_outputs(const SandiLongArgs &a, int v)
{
    const double nan = __builtin_nan("");
    for (int m = 0; m < 6; m++) a.est[(size_t)v * 6 + m] = nan;
    if (a.rmse) a.rmse[v] = nan;
    if (a.nrmse) a.nrmse[v] = nan;
}

template <int N>
__global__ void __launch_bounds__(256) k_sandi_gram_lane(const SandiLongArgs a)
{
    __shared__ double Hs[N * N], Gs[N * N], s_par[2][16];
    const int n_atoms = a.n_atoms, n_rs = a.n_rs, n_in = a.n_in, NP = a.NP;
    for (int e = threadIdx.x; e < N * N; e += (int)blockDim.x) {
        const int j = e / N, k = e - j * N;
        Hs[e] = a.H[j * NP + k]; Gs[e] = a.G[j * NP + k];
    }
    if (threadIdx.x < 16) {
        const int j = threadIdx.x;
        s_par[0][j] = j < n_atoms ? a.norms[j] : 0.0;
        s_par[1][j] = j < n_rs ? a.Rs[j] : (j < n_rs + n_in ? a.d_in[j - n_rs] : (j < n_atoms ? a.d_isos[j - n_rs - n_in] : 0.0));
    }
    __syncthreads();
    const int v = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (v >= a.n) return;
    const double *src = a.Cb + (size_t)(v >> 6) * a.rows * 64 + (v & 63);      // the voxel's column of its block: coalesced over the lanes
    double c[N], x[N];
#pragma unroll
    for (int j = 0; j < N; j++) c[j] = src[(size_t)j * 64];                    // (rows of the padding atoms are zero)
    const double ysq = src[(size_t)NP * 64];
    if (src[(size_t)(NP + 1) * 64] == 0.0) { sl_nan_outputs(a, v); return; }   // a non-finite sample
#pragma unroll
    for (int j = 0; j < N; j++) c[j] -= a.lam1;
    if (lane_nnqp<N>(Hs, c, x, n_atoms, amx_warm_start(a.lam2, a.flags)) != 0) atomicAdd(&a.status[ST_ITCAP], 1);
    // models.pyx:1570-1612
    double x_sum = 0.0, xsph = 0.0, xstk = 0.0, xiso = 0.0, Rsoma = 0.0, Din = 0.0, De = 0.0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const double nj = s_par[0][j], pj = s_par[1][j];
        if (j < n_atoms) {
            x[j] *= nj;
            x_sum += x[j];
            if (j < n_rs) { xsph += x[j]; Rsoma += pj * x[j]; }
            else if (j < n_rs + n_in) { xstk += x[j]; Din += pj * x[j]; }
            else { xiso += x[j]; De += pj * x[j]; }
        } else x[j] = 0.0;
    }
    if (a.xdbg) {                                         // the rescaled x (models.pyx:1570-1571)
#pragma unroll
        for (int j = 0; j < N; j++) if (j < n_atoms) a.xdbg[(size_t)v * n_atoms + j] = x[j];
    }
    double *e = a.est + (size_t)v * 6;
    x_sum += 1e-16;
    e[0] = fast_div(xsph, x_sum); e[1] = fast_div(xstk, x_sum); e[2] = fast_div(xiso, x_sum);
    e[3] = 1e6 * fast_div(Rsoma, xsph + 1e-16);
    e[4] = 1e3 * fast_div(Din, xstk + 1e-16);
    e[5] = 1e3 * fast_div(De, xiso + 1e-16);
    if (a.rmse || a.nrmse) {
        // quirk kept (models.pyx:1571 then 1615): errors use the RESCALED x with the NORMALISED A -- through the Gram identity, with the raw c
        AMX_RELOAD();
        double xc = 0.0, xgx = 0.0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < N; k++) t += Gs[j * N + k] * x[k];
            xgx += x[j] * t;
            xc += x[j] * src[(size_t)j * 64];
        }
        double rss = ysq - 2.0 * xc + xgx;
        rss = rss > 0.0 ? rss : 0.0;
        if (a.rmse) a.rmse[v] = sqrt(rss / (double)a.nS);
        if (a.nrmse) a.nrmse[v] = (ysq > 1e-16) ? sqrt(rss / ysq) : 0.0;
    }
}

__device__ __forceinline__ int sl_tri(int r, int s) { return r * (r + 1) / 2 + s; }

// One 64-thread workgroup per voxel, lane = atom.  min 1/2 x'Hx - (c - lambda1)'x, x >= 0, strictly convex: block principal pivoting from
// the full set -- solve H_PP z = c_P by a dense Cholesky factorisation, dual values g = c - H z off P, exchange ALL infeasible atoms while
// their number keeps falling (then kBackup more times), else the one with the largest index (Murty: finite for a positive definite H).
__global__ void __launch_bounds__(64) k_sandi_gram_wave(const SandiLongArgs a)
{
    __shared__ double L[64 * 65 / 2], cv[64], zv[64], zat[64];
    __shared__ int plist[64], inP[64], bad[64], shi[4];      // shi: 0 np, 1 n_bad, 2 largest bad atom, 3 pivot failure
    const int n = a.n_atoms, NP = a.NP, lane = threadIdx.x, n_rs = a.n_rs, n_in = a.n_in;
    const double *H = a.H, *G = a.G;
    const bool at = lane < n;
    const bool sph = at && lane < n_rs, stk = at && !sph && lane < n_rs + n_in, iso = at && !sph && !stk;
    const double nj = at ? a.norms[lane] : 0.0;
    const double pj = sph ? a.Rs[lane] : (stk ? a.d_in[lane - n_rs] : (iso ? a.d_isos[lane - n_rs - n_in] : 0.0));
    constexpr int kBackup = 3;
    for (int v = blockIdx.x; v < a.n; v += (int)gridDim.x) {
        const double *src = a.Cb + (size_t)(v >> 6) * a.rows * 64 + (v & 63);
        const double craw = at ? src[(size_t)lane * 64] : 0.0;
        const double ysq = src[(size_t)NP * 64];
        if (src[(size_t)(NP + 1) * 64] == 0.0) {                 // a non-finite sample (uniform over the workgroup)
            if (lane == 0) sl_nan_outputs(a, v);
            continue;
        }
        // the dual tests compare gradients (units of c) with zero: the tolerance follows the voxel's own scale (k_czb_lane)
        const double cmax = amx::wave_max(fabs(craw));
        const double tol = 1e-12 * cmax;
        __syncthreads();
        cv[lane] = craw - a.lam1; zat[lane] = 0.0; inP[lane] = at ? 1 : 0; bad[lane] = 0;
        if (lane < 4) shi[lane] = 0;
        __syncthreads();
        int ninf = n + 1, backup = 0, status = kSolved;
        for (int step = 0;; ++step) {
            if (step > 4 * n + 16) { status = kIterCap; break; }
            // ---- P in ascending order
            if (at && inP[lane]) {
                int r = 0;
                for (int k = 0; k < lane; k++) r += inP[k];
                plist[r] = lane;
            }
            if (lane == 0) { int c2 = 0; for (int k = 0; k < n; k++) c2 += inP[k]; shi[0] = c2; shi[1] = 0; shi[2] = -1; }
            __syncthreads();
            const int np = shi[0];
            // ---- H_PP (packed lower triangle) and the right-hand side
            if (lane < np) {
                const int pr = plist[lane];
                const double *Hr = H + (size_t)pr * NP;
                for (int s = 0; s <= lane; s++) L[sl_tri(lane, s)] = Hr[plist[s]];
                zv[lane] = cv[pr];
            }
            __syncthreads();
            // ---- Cholesky in place, right-looking (lambda2 > 0: every pivot >= lambda2)
            for (int k = 0; k < np; k++) {
                const double dk = L[sl_tri(k, k)];
                if (!(dk > 0.0)) { if (lane == 0) shi[3] = 1; break; }
                const double d = sqrt(dk), di = 1.0 / d;
                __syncthreads();
                if (lane >= k && lane < np) L[sl_tri(lane, k)] = (lane == k) ? d : L[sl_tri(lane, k)] * di;
                __syncthreads();
                for (int r = k + 1 + (lane >> 3); r < np; r += 8) {          // 8 x 8 threads over the trailing triangle
                    const double lrk = L[sl_tri(r, k)];
                    for (int s = k + 1 + (lane & 7); s <= r; s += 8) L[sl_tri(r, s)] -= lrk * L[sl_tri(s, k)];
                }
                __syncthreads();
            }
            __syncthreads();
            if (shi[3]) { status = kGuardOuter; break; }
            // ---- L w = c_P, L'z = w (column oriented: one step per pivot)
            for (int k = 0; k < np; k++) {
                const double wk = zv[k] / L[sl_tri(k, k)];
                __syncthreads();
                if (lane == 0) zv[k] = wk;
                if (lane > k && lane < np) zv[lane] -= L[sl_tri(lane, k)] * wk;
                __syncthreads();
            }
            for (int k = np - 1; k >= 0; k--) {
                const double zk = zv[k] / L[sl_tri(k, k)];
                __syncthreads();
                if (lane == 0) zv[k] = zk;
                if (lane < k) zv[lane] -= L[sl_tri(k, lane)] * zk;
                __syncthreads();
            }
            zat[lane] = 0.0;
            __syncthreads();
            if (lane < np) zat[plist[lane]] = zv[lane];
            __syncthreads();
            // ---- infeasible atoms: passive with z <= 0, inactive with a positive dual value g_j = c_j - sum_s H_js z_s
            bool viol = false;
            if (at) {
                if (inP[lane]) viol = !(zat[lane] > 0.0);
                else {
                    const double *Hj = H + (size_t)lane * NP;
                    double g = 0.0;
                    for (int r = 0; r < np; r++) g += Hj[plist[r]] * zv[r];
                    viol = (cv[lane] - g) > tol;
                }
            }
            bad[lane] = viol ? 1 : 0;
            if (viol) { atomicAdd(&shi[1], 1); atomicMax(&shi[2], lane); }
            __syncthreads();
            const int nbad = shi[1], top = shi[2];
            if (nbad == 0) break;                                   // Kuhn-Tucker point of a strictly convex problem: the optimum
            bool block = false;
            if (nbad < ninf) { ninf = nbad; backup = kBackup; block = true; }
            else if (backup > 0) { backup--; block = true; }
            __syncthreads();
            if (at && (block ? bad[lane] != 0 : lane == top)) inP[lane] ^= 1;
            __syncthreads();
        }
        if (status == kIterCap && lane == 0) atomicAdd(&a.status[ST_ITCAP], 1);
        if (status > kIterCap && lane == 0) { atomicAdd(&a.status[ST_GUARD], 1); a.status[ST_GUARDVOX] = v * 8 + status; }
        // models.pyx:1570-1612 (a clamped or infeasible iterate never reaches the maps negative)
        const double xs = (at && inP[lane] && zat[lane] > 0.0) ? zat[lane] * nj : 0.0;
        if (a.xdbg && at) a.xdbg[(size_t)v * n + lane] = xs;
        const double x_sum = amx::wave_sum(xs) + 1e-16;
        const double xsph = amx::wave_sum(sph ? xs : 0.0), xstk = amx::wave_sum(stk ? xs : 0.0), xiso = amx::wave_sum(iso ? xs : 0.0);
        const double Rsoma = amx::wave_sum(sph ? pj * xs : 0.0), Din = amx::wave_sum(stk ? pj * xs : 0.0), De = amx::wave_sum(iso ? pj * xs : 0.0);
        if (lane == 0) {
            double *e = a.est + (size_t)v * 6;
            e[0] = xsph / x_sum; e[1] = xstk / x_sum; e[2] = xiso / x_sum;
            e[3] = 1e6 * Rsoma / (xsph + 1e-16);
            e[4] = 1e3 * Din / (xstk + 1e-16);
            e[5] = 1e3 * De / (xiso + 1e-16);
        }
        if (a.rmse || a.nrmse) {
            // quirk kept (models.pyx:1571 then 1615): the RESCALED x with the NORMALISED A, through rss = y'y - 2 x'c + x'G x
            __syncthreads();
            zv[lane] = xs;
            __syncthreads();
            double t = 0.0;
            if (at) { const double *Gj = G + (size_t)lane * NP; for (int k = 0; k < n; k++) t += Gj[k] * zv[k]; }
            double rss = ysq + amx::wave_sum(xs * (t - 2.0 * craw));
            rss = rss > 0.0 ? rss : 0.0;
            if (lane == 0) {
                if (a.rmse) a.rmse[v] = sqrt(rss / (double)a.nS);
                if (a.nrmse) a.nrmse[v] = (ysq > 1e-16) ? sqrt(rss / ysq) : 0.0;
            }
        }
    }
}

// (sl_ksteps, sl_padded_atoms: amx_small_route.hpp)
template <int N>
void launch_gram_lane(const SandiLongArgs &f, hipStream_t s) { hipLaunchKernelGGL(k_sandi_gram_lane<N>, dim3((f.n + 255) / 256), dim3(256), 0, s, f); }

}  // namespace

// doubles of the cached tables (amx_debug_fetch)
size_t amx_sandi_long_table_words(const amx_lut *lut)
{
    const int NP = sl_padded_atoms(lut->n_atoms), KS = sl_ksteps(lut->nS);
    return (size_t)2 * NP * NP + (size_t)(NP / 16) * KS * 64;
}

// G, H and the operand A' of one dictionary and one lambda2, cached in the dictionary handle
int amx_sandi_long_prepare(amx_ctx *ctx, const amx_lut *lut, double lam2, hipStream_t s)
{
    const int NP = sl_padded_atoms(lut->n_atoms), KS = sl_ksteps(lut->nS);
    if (lut->sandi_long_lam2 != lam2 || !lut->sandi_long_prep) {
        if (lut->sandi_long_prep) HIPCHK(ctx, hipDeviceSynchronize());                          // (a fit with the old tables may still run)
        if (!lut->sandi_long_prep) HIPCHK(ctx, hipMalloc((void **)&lut->sandi_long_prep, amx_sandi_long_table_words(lut) * sizeof(double)));
        if (!lut->sandi_long_ready) HIPCHK(ctx, hipEventCreateWithFlags(&lut->sandi_long_ready, hipEventDisableTiming));
        hipLaunchKernelGGL(k_sandi_long_tables, dim3(16), dim3(256), 0, s, reinterpret_cast<const double *>(lut->tiles), lut->nS, lut->ldA, lut->n_atoms,
                           lam2, NP, KS, lut->sandi_long_prep);
        AMX_TRACE(ctx, s, "SANDI Gram tables (G, H, A' in MFMA order)");
        HIPCHK(ctx, hipEventRecord(lut->sandi_long_ready, s));
        lut->sandi_long_lam2 = lam2;
    }
    HIPCHK(ctx, hipStreamWaitEvent(s, lut->sandi_long_ready, 0));
    return AMX_OK;
}

// the voxels in order (one dictionary: no plan); counts straight into the status words
int amx_launch_sandi_long(amx_ctx *ctx, const amx_lut *lut, const SandiArgs &a, int64_t n, hipStream_t s, const SmallRoute &rt)
{
    SandiLongArgs f;
    memset(&f, 0, sizeof f);
    f.y = a.c.y; f.y32 = a.c.y32; f.n = (int)n; f.nS = lut->nS; f.n_atoms = lut->n_atoms; f.n_rs = a.n_rs; f.n_in = a.n_in;
    f.NP = sl_padded_atoms(lut->n_atoms); f.ksteps = sl_ksteps(lut->nS); f.rows = f.NP + 2;
    f.G = lut->sandi_long_prep; f.H = f.G + f.NP * f.NP; f.At = f.H + f.NP * f.NP;
    f.norms = a.norms; f.Rs = a.Rs; f.d_in = a.d_in; f.d_isos = a.d_isos;
    f.lam1 = a.c.lam1; f.lam2 = a.c.lam2; f.flags = a.c.flags;
    f.est = a.est; f.rmse = a.rmse; f.nrmse = a.nrmse; f.xdbg = a.c.xdbg; f.status = a.c.status;
    const int n_blk = (int)((n + 63) / 64);
    int rc;
    if ((rc = amx_ensure(ctx, ctx->cgemm, (size_t)n_blk * f.rows * 64 * sizeof(double)))) return rc;
    f.Cb = (double *)ctx->cgemm.p;
    const size_t lds = rt.lds;              // (the A' operand of one atom tile: ksteps x 64 doubles)
    const int per_cu = (int)(kLdsPerCU / lds) < 8 ? (int)(kLdsPerCU / lds) : 8;      // (8 workgroups of 4 wavefronts fill a CU)
    const int grid = n_blk < ctx->n_cu * per_cu ? n_blk : ctx->n_cu * per_cu;
    rec(ctx, 4, s);                          // (amx_last_kernel_ms: 2 = the projection, 1 = the solver)
    if (f.y32) rc = launch_lds(ctx, k_sandi_project<float>, dim3(grid), dim3(256), lds, s, f);
    else rc = launch_lds(ctx, k_sandi_project<double>, dim3(grid), dim3(256), lds, s, f);
    if (rc) return rc;
    amx_note(ctx, rt.launch[0]);
    AMX_TRACE(ctx, s, "c = A'y, y'y on the matrix cores");
    rec(ctx, 5, s);
    rec(ctx, 2, s);
    if (rt.family == SF_SANDI_LONG_LANE) {
        if (rt.N == 12) launch_gram_lane<12>(f, s);
        else if (rt.N == 15) launch_gram_lane<15>(f, s);
        else launch_gram_lane<16>(f, s);
        amx_note(ctx, rt.launch[1]);
        AMX_TRACE(ctx, s, "Gram-space solver, one voxel per lane");
    } else {
        const int64_t cap = (int64_t)ctx->n_cu * 16;
        hipLaunchKernelGGL(k_sandi_gram_wave, dim3((unsigned)(n < cap ? n : cap)), dim3(64), 0, s, f);
        amx_note(ctx, rt.launch[1]);
        AMX_TRACE(ctx, s, "Gram-space solver, one wavefront per voxel");
    }
    rec(ctx, 3, s);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}
