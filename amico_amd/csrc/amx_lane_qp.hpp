// amx_lane_qp.hpp -- the per-lane solver of the FreeWater / SANDI fits for small dictionaries (n_atoms <= 16): ONE VOXEL PER LANE.
//
// models.pyx:1231-1276 (FreeWater) and :1567-1619 (SANDI) solve, per voxel,
//     min_x 1/2||y - A x||^2 + lambda1*sum(x) + lambda2/2*||x||^2 ,  x >= 0      (cyspams lasso)
// with 11..15 atoms and lambda2 > 0.  A wavefront per voxel (amx_solver.hpp) leaves most lanes idle
// on such problems, so the kernels of amx_fw_lane.hip and amx_sandi_lane.hip map one voxel to one LANE:
//   * the workgroup's voxels share one orientation (bucketing) => A (nS x n) and the regularised
//     Gram matrix H = A'A + lambda2*I (n x n, built by the workgroup itself in its prologue) sit in
//     LDS and are read with wave-uniform (broadcast) addresses;
//   * each lane forms c = A'y from its own signal row and runs a Lawson-Hanson active set on
//     (H, c) entirely in registers: the passive set is a bit mask, the passive system is solved by a
//     MASKED Cholesky factorisation (rows/columns outside the set replaced by identity), all loops
//     are fully unrolled over the compile-time dictionary size => no cross-lane traffic, and lane
//     divergence is plain SIMT predication.
// H is well conditioned thanks to the ridge (cond <= ~1e6 for AMICO's defaults), so Gram space is
// safe here (it is NOT for NODDI's unregularised NNLS stages).
// Here: what the two units share -- the per-lane solver (lane_solve, lane_nnqp), the workgroup prologue (small_prologue), A'y and
// the residual per lane, and launch_lane, the host function that launches a lane kernel of either.  Each unit is compiled on its
// own: the anonymous namespace keeps a copy per unit.
#pragma once
#include "amx_launch.hpp"
using namespace amx;

namespace {

template <int N>
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

// x / d for well-scaled operands (no denormal / overflow handling: v_rcp_f64, two Newton steps, one residual correction;
// ~9 instructions against ~35 of the IEEE sequence, within 1 ulp)
__device__ __forceinline__ double fast_div(double x, double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    const double q = x * r;
    return __builtin_fma(__builtin_fma(-d, q, x), r, q);
}

// H / the dictionary are loop invariant: without these barriers the compiler keeps their entries in vector registers
// across the fully unrolled passes (hundreds of VGPRs) and spills everything else
#define AMX_RELOAD() asm volatile("" ::: "memory")

// Cholesky of H restricted to P and the two triangular solves: z = H_PP^-1 cc_P (0 elsewhere).
// The restriction costs ONE select per column: ivm_j = 1 / L_jj for j in P, 0 otherwise.  A zero ivm_j zeroes column j of
// the factor (so no row of P ever sees atom j) and z_j in both substitutions.  Row j itself is then computed from whatever
// the arithmetic gives (finite: sums of products of bounded entries; a negative pivot only feeds the discarded rsqrt) --
// nothing reads it, because every use of row j is multiplied by ivm_j or by z_j = 0.
template <int N>
__device__ __forceinline__ void lane_solve(const double *__restrict__ Hs, const double (&cc)[N], unsigned P, double (&z)[N])
{
    double L[N * (N + 1) / 2], ivm[N];
    AMX_RELOAD();
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = Hs[j * N + j];
#pragma unroll
        for (int k = 0; k < j; k++) s -= L[tri<N>(j, k)] * L[tri<N>(j, k)];
        const double iv = ((P >> j) & 1u) ? rsqrt(s) : 0.0;
        ivm[j] = iv;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double tt = Hs[i * N + j];
#pragma unroll
            for (int k = 0; k < j; k++) tt -= L[tri<N>(i, k)] * L[tri<N>(j, k)];
            L[tri<N>(i, j)] = tt * iv;
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = cc[j];
#pragma unroll
        for (int k = 0; k < j; k++) s -= L[tri<N>(j, k)] * z[k];
        z[j] = s * ivm[j];
    }
#pragma unroll
    for (int j = N - 1; j >= 0; j--) {
        double s = z[j];
#pragma unroll
        for (int i = j + 1; i < N; i++) s -= L[tri<N>(i, j)] * z[i];
        z[j] = s * ivm[j];
    }
}

// per-lane NNQP: min 1/2 x'Hx - cc'x, x >= 0 (cc = c - lambda1); Hs in LDS, row-major N x N.
// warm: start from all n_atoms atoms and drop the non-positive ones in blocks before the Lawson-Hanson loop takes over
// (unique optimum with the ridge; see lane_nnqp_rows).  returns 0, or 2 if an iteration cap tripped.
template <int N>
__device__ __forceinline__ int lane_nnqp(const double *__restrict__ Hs, const double (&cc)[N], double (&x)[N],
                                         int n_atoms = N, bool warm = false)
{
    const double inf = __builtin_huge_val();
    double z[N];
    unsigned P = 0u;
    int status = 0;
    // the dual test compares gradients (units of cc) with zero: its tolerance follows the voxel's own scale, so that a voxel of
    // amplitude 2^-20 is solved as far as one of amplitude 1 (1e-12 as it has always been where max |cc| >= 1)
    double cmax = 0.0;
#pragma unroll
    for (int j = 0; j < N; j++) { x[j] = 0.0; cmax = fmax(cmax, fabs(cc[j])); }
    const double tol = 1e-12 * fmin(cmax, 1.0);
    if (warm) {
        P = (1u << n_atoms) - 1u;
        for (int round = 0; round < N && P != 0u; ++round) {
            lane_solve<N>(Hs, cc, P, z);
            unsigned negm = 0u;
#pragma unroll
            for (int j = 0; j < N; j++)
                if (((P >> j) & 1u) && !(z[j] > 0.0)) negm |= 1u << j;
            if (negm == 0u) {
#pragma unroll
                for (int j = 0; j < N; j++) x[j] = ((P >> j) & 1u) ? z[j] : 0.0;
                break;
            }
            P &= ~negm;
        }
    }
    for (int it = 0; status == 0; ++it) {
        if (it > 3 * N + 8) { status = 2; break; }
        // dual vector g = cc - H x, most violating atom outside the passive set
        AMX_RELOAD();
        double best = -inf;
        int t = -1;
#pragma unroll
        for (int j = 0; j < N; j++) {
            double g = cc[j];
#pragma unroll
            for (int k = 0; k < N; k++) g -= Hs[j * N + k] * x[k];
            if (!((P >> j) & 1u) && g > best) { best = g; t = j; }
        }
        if (!(best > tol)) break;               // KKT point
        P |= 1u << t;
        for (int in = 0;; ++in) {
            if (in > N + 2) { status = 2; break; }
            lane_solve<N>(Hs, cc, P, z);
            bool feasible = true;
#pragma unroll
            for (int j = 0; j < N; j++)
                if (((P >> j) & 1u) && !(z[j] > 0.0)) feasible = false;
            if (feasible) {
#pragma unroll
                for (int j = 0; j < N; j++) x[j] = ((P >> j) & 1u) ? z[j] : 0.0;
                break;
            }
            double alpha = inf;
            int jm = -1;
#pragma unroll
            for (int j = 0; j < N; j++) {
                if (((P >> j) & 1u) && !(z[j] > 0.0)) {
                    const double den = x[j] - z[j];
                    const double r = (den > 0.0) ? x[j] / den : 0.0;
                    if (r < alpha) { alpha = r; jm = j; }
                }
            }
#pragma unroll
            for (int j = 0; j < N; j++) {
                if ((P >> j) & 1u) {
                    x[j] += alpha * (z[j] - x[j]);
                    if (j == jm || !(x[j] > 0.0)) { x[j] = 0.0; P &= ~(1u << j); }
                }
            }
            if (P == 0u) break;
        }
    }
    return status;
}

// workgroup prologue: tile -> LDS, H = A'A + lambda2*I (identity on the padding atoms)
template <int N, typename AT>
__device__ __forceinline__ void small_prologue(const AT *__restrict__ tile, int words, AT *As, double *Hs, int nS,
                                               int ldA, int n_atoms, double lam2)
{
    for (int k = threadIdx.x; k < words; k += blockDim.x) As[k] = tile[k];
    __syncthreads();
    for (int e = threadIdx.x; e < N * N; e += blockDim.x) {
        const int j = e / N, k = e % N;
        double acc = (j == k) ? ((j < n_atoms) ? lam2 : 1.0) : 0.0;
        if (j < n_atoms && k < n_atoms)
            for (int i = 0; i < nS; i++) acc += (double)As[i * ldA + j] * (double)As[i * ldA + k];
        Hs[e] = acc;
    }
    __syncthreads();
}

// c = A'y for this lane's voxel (+ sum y^2); A read with wave-uniform LDS addresses
template <int N, typename AT>
__device__ __forceinline__ bool lane_aty(const AT *As, const double *__restrict__ yv, int nS, int ldA, int n_atoms,
                                         double (&c)[N], double &ysq)
{
    bool finite = true;
    ysq = 0.0;
#pragma unroll
    for (int j = 0; j < N; j++) c[j] = 0.0;
    // the lane's signal row is strided in memory (one cache line per lane and load): keep sixteen loads in flight
    int i = 0;
    for (; i + 16 <= nS; i += 16) {
        double yb[16];
#pragma unroll
        for (int u = 0; u < 16; u++) yb[u] = yv[i + u];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const double yi = yb[u];
            finite = finite && (fabs(yi) <= 1.79769313486231570e308);
            ysq += yi * yi;
#pragma unroll
            for (int j = 0; j < N; j++)
                if (j < n_atoms) c[j] += (double)As[(i + u) * ldA + j] * yi;
        }
    }
    for (; i < nS; i++) {
        const double yi = yv[i];
        finite = finite && (fabs(yi) <= 1.79769313486231570e308);
        ysq += yi * yi;
#pragma unroll
        for (int j = 0; j < N; j++)
            if (j < n_atoms) c[j] += (double)As[i * ldA + j] * yi;
    }
    return finite;
}

template <int N, typename AT>
__device__ __forceinline__ double lane_rss(const AT *As, const double *__restrict__ yv, int nS, int ldA, int n_atoms,
                                           const double (&x)[N])
{
    double rss = 0.0;
    for (int i = 0; i < nS; i++) {
        double e = yv[i];
#pragma unroll
        for (int j = 0; j < N; j++)
            if (j < n_atoms) e -= (double)As[i * ldA + j] * x[j];
        rss += e * e;
    }
    return rss;
}

#define AMX_SMALL_LDS(AT)                                                                        \
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];                      \
    const int words = a.c.nS * a.c.ldA;                                                          \
    AT *As = reinterpret_cast<AT *>(smem_s);                                                     \
    double *Hs = reinterpret_cast<double *>(smem_s + (((size_t)words * sizeof(AT) + 15) & ~(size_t)15));

// (the LDS -- lane_lds_bytes, amx_sizes.hpp -- and the note are the route's)
template <typename Args, typename K>
int launch_lane(amx_ctx *ctx, Args &a, const Plan &pl, hipStream_t s, K kern, const amx::SmallRoute &rt)
{
    const size_t lds = rt.lds;
    int rc;
    if ((rc = set_lds(ctx, kern, lds))) return rc;
    rec(ctx, 2, s);
    hipLaunchKernelGGL(kern, dim3(((pl.max_chunks + 7) / 8) * 8), dim3(256), lds, s, a);
    amx_note(ctx, rt.launch[0]);
    AMX_TRACE(ctx, s, "lane-per-voxel solver");
    rec(ctx, 3, s);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

}  // namespace
