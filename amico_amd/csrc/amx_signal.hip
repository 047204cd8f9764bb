// amx_signal.hip -- the steps either side of model.fit (SURVEY section 8 f): principal directions from the
// log-linear tensor fit (core.py:431-436, 456-458) -- streaming, HBM-bound kernels -- and from the weighted / non-linear
// fits of DTI_fit_method 'WLS' / 'NLLS' and the robust fit 'RT' / 'RESTORE' (core.py:419-420, 436), k_dti_dirs_w.
#include "amx_host.hpp"
#include "amx_tensor.hpp"

using namespace amx;

namespace amx {

constexpr int kDtiVox = 64;                 // voxels per tile
constexpr int kDtiLanes = 8;                // lanes sharing one voxel's contraction
constexpr int kDtiThreads = kDtiLanes * kDtiVox;
constexpr int kDtiBatch = 4;                // tiles whose tensors are diagonalised together (one per lane, 4 wavefronts)

// y f64[n][nS] -> dirs f64[n][3].  Tiles of `tv` voxels (tv * nS <= kDtiPre * 2 * kDtiThreads doubles):
// (1) the tile is streamed with 16-byte lane loads into registers one tile AHEAD of its use, so that the HBM
// latency is covered by the arithmetic of the previous tile; (2) log(max(y, min_signal)) (TensorModel.fit +
// ols_fit_tensor, dipy/reconst/dti.py) goes to LDS; (3) kDtiLanes lanes per voxel contract the log-signal with the
// first six rows of pinv(design matrix) (LDS, [nS][6]); (4) every kDtiBatch tiles, wavefronts 0..3 (one per SIMD)
// diagonalise the batch's tensors, one per lane -- the Jacobi sweeps are a serial chain, so they are batched to
// full wavefronts and spread over the SIMDs instead of being left to one wavefront per tile.
constexpr int kDtiPre = 8;                  // double2 registers per thread holding the tile in flight

__device__ __forceinline__ void dti_prefetch(double2 (&pre)[kDtiPre], const double *__restrict__ src, int cnt, int tid)
{
#pragma unroll
    for (int i = 0; i < kDtiPre; i++) {
        const int e = 2 * (tid + i * kDtiThreads);
        if (e + 1 < cnt) pre[i] = *reinterpret_cast<const double2 *>(src + e);
        else if (e < cnt) pre[i] = make_double2(src[e], 1.0);
    }
}
// float32 signals (the image's own dtype, core.py:136): two 4-byte loads per pair (a tile starts at any multiple of 4 bytes)
__device__ __forceinline__ void dti_prefetch(double2 (&pre)[kDtiPre], const float *__restrict__ src, int cnt, int tid)
{
    // (loads under their guards, conversions outside them: converted inside its guard, every load was waited for before the next one left)
    float r0[kDtiPre], r1[kDtiPre];
#pragma unroll
    for (int i = 0; i < kDtiPre; i++) {
        const int e = 2 * (tid + i * kDtiThreads);
        r0[i] = 1.0f; r1[i] = 1.0f;
        if (e < cnt) r0[i] = src[e];
        if (e + 1 < cnt) r1[i] = src[e + 1];
    }
#pragma unroll
    for (int i = 0; i < kDtiPre; i++) {
        const int e = 2 * (tid + i * kDtiThreads);
        if (e < cnt) pre[i] = make_double2((double)r0[i], (double)r1[i]);
    }
}

// The end of every tensor kernel: the thread's tensor of the batch -> its outputs.  MAPS = false is the principal direction alone.
// MAPS = true (amx_dti_fit*): besides, evals f64[n][3] -- descending, clipped from below at min_diffusivity as dipy's
// decompose_tensor does for TensorModel -- and scalars f64[n][4] = FA, MD, AD, RD of the clipped eigenvalues; each of the three
// outputs may be null.
template <bool MAPS>
__device__ __forceinline__ void dti_store(const double (&d)[6], long long v, double *__restrict__ dirs, double min_diffusivity,
                                          double *__restrict__ evals, double *__restrict__ scalars)
{
    double o[3];
    if constexpr (MAPS) {
        double e[3], sc[4];
        tensor_eigen(d, e, o);
        tensor_scalars(e, min_diffusivity, sc);
        if (evals) { double *dst = evals + v * 3; dst[0] = e[0]; dst[1] = e[1]; dst[2] = e[2]; }
        if (scalars) { double *dst = scalars + v * 4; dst[0] = sc[0]; dst[1] = sc[1]; dst[2] = sc[2]; dst[3] = sc[3]; }
        if (!dirs) return;
    } else {
        principal_direction(d, o);
    }
    double *dst = dirs + v * 3;
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

template <typename YT, bool MAPS>
__global__ __launch_bounds__(kDtiThreads, 4) void k_dti_dirs(const YT *__restrict__ y, const double *__restrict__ wt,
                                                         int nS, int ldl, int tv, long long n, double min_signal,
                                                         double *__restrict__ dirs, double min_diffusivity,
                                                         double *__restrict__ evals, double *__restrict__ scalars)
{
    extern __shared__ double sm[];
    double *wl = sm;                                   // nS * 6
    double *yl = sm + ((nS * 6 + 1) & ~1);             // tv * ldl
    double *dl = yl + tv * ldl;                        // kDtiBatch * tv * 7 (6 tensor entries, odd stride)
    const int tid = threadIdx.x;
    for (int i = tid; i < nS * 6; i += kDtiThreads) wl[i] = wt[i];
    const long long n_tiles = (n + tv - 1) / tv;
    const int step = 2 * kDtiThreads;
    const int step_vol = step % nS, step_adr = (step / nS) * ldl + step_vol;
    const int vox0 = (2 * tid) / nS, vol0 = 2 * tid - vox0 * nS, adr0 = vox0 * ldl + vol0;
    const int eslot = tid / tv, evox = tid - eslot * tv;      // tensor this thread diagonalises in a batch
    double2 pre[kDtiPre];
#pragma unroll
    for (int i = 0; i < kDtiPre; i++) pre[i] = make_double2(1.0, 1.0);
    long long tile = blockIdx.x;
    if (tile < n_tiles) {
        const long long v0 = tile * tv;
        dti_prefetch(pre, y + v0 * nS, (int)((n - v0) < tv ? (n - v0) : tv) * nS, tid);
    }
    long long batch_tile = tile;                       // first tile of the batch being collected
    int slot = 0;
    for (; tile < n_tiles; tile += gridDim.x) {
        const long long v0 = tile * tv;
        const int nv = (int)((n - v0) < tv ? (n - v0) : tv);
        const int cnt = nv * nS;
#pragma unroll
        for (int i = 0; i < kDtiPre; i++) {            // independent chains: no guards, so that they interleave
            pre[i].x = fast_log(fmax(pre[i].x, min_signal));
            pre[i].y = fast_log(fmax(pre[i].y, min_signal));
        }
        int vol = vol0, adr = adr0;
#pragma unroll
        for (int i = 0; i < kDtiPre; i++) {
            const int e = 2 * (tid + i * kDtiThreads);
            if (e < cnt) yl[adr] = pre[i].x;
            if (e + 1 < cnt) yl[vol + 1 == nS ? adr + 1 + ldl - nS : adr + 1] = pre[i].y;
            vol += step_vol; adr += step_adr;
            if (vol >= nS) { vol -= nS; adr += ldl - nS; }
        }
        __syncthreads();                               // log-signals of this tile are in LDS
        const long long nt = tile + gridDim.x;
        if (nt < n_tiles) {
            const long long w0 = nt * tv;
            dti_prefetch(pre, y + w0 * nS, (int)((n - w0) < tv ? (n - w0) : tv) * nS, tid);
        }
        const int vox = tid / kDtiLanes, q = tid % kDtiLanes;
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (vox < nv) {
            const double *yr = yl + vox * ldl;
            for (int v = q; v < nS; v += kDtiLanes) {
                const double ly = yr[v];
                const double *w = wl + v * 6;
#pragma unroll
                for (int k = 0; k < 6; k++) acc[k] = fma(w[k], ly, acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 6; k++) {
#pragma unroll
            for (int m = 1; m < kDtiLanes; m <<= 1) acc[k] += __shfl_xor(acc[k], m);
        }
        if (q == 0 && vox < nv) {
#pragma unroll
            for (int k = 0; k < 6; k++) dl[(slot * tv + vox) * 7 + k] = acc[k];
        }
        slot++;
        __syncthreads();                               // tensors in LDS; the log-signal rows may be overwritten
        if (slot == kDtiBatch || nt >= n_tiles) {
            if (eslot < slot) {
                const long long e0 = (batch_tile + (long long)eslot * gridDim.x) * tv;
                if (e0 + evox < n) {
                    double d[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) d[k] = dl[(eslot * tv + evox) * 7 + k];
                    dti_store<MAPS>(d, e0 + evox, dirs, min_diffusivity, evals, scalars);
                }
            }
            slot = 0;
            batch_tile = nt;
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------
// WLS and NLLS tensor fits (dipy/reconst/dti.py: wls_fit_tensor, nlls_fit_tensor with weighting=None).  X = design matrix
// [nS][7], s = max(y, min_signal):
//   WLS   p_ols = pinv(X) log s;  w = exp(X p_ols) (the signal OLS predicts);  p = argmin sum w_i^2 (log s_i - X_i p)^2
//         (dipy: pinv(X * w[:, None]) @ (w * log s))
//   NLLS  p = argmin sum (s_i - exp(X_i p))^2: the local minimum next to the linear fit.  dipy runs MINPACK's
//         Levenberg-Marquardt from a linear fit (which one has changed between dipy releases; the minimum does not depend on it
//         except in pathological voxels) and keeps the starting parameters when the solve fails.  Here: Levenberg-Marquardt
//         from the WLS solution, stopped when the cost no longer moves in fp64.
// Both run on the design matrix with its columns scaled to unit max-abs (host side; the scale is undone on the six tensor
// entries before the eigen-solve): the 7 x 7 normal matrix of the scaled system is conditioned well enough for a register
// Cholesky to reproduce the SVD route (cond(X) = 2.1e3 on the 99-volume scheme, cond of the scaled normal matrix <= 2.5e2).
//
// Tile staging, logarithms and the batched eigen-solves are k_dti_dirs'.  In between, the eight lanes of a voxel each
// accumulate their share of the 28 + 7 normal-equation sums over the voxel's LDS row; an xor-butterfly leaves all eight with
// the same bits, and all eight run the 7 x 7 Cholesky solve redundantly -- no LDS round trip or barrier inside the
// Levenberg-Marquardt loop, and a wavefront waits for the slowest of its 8 voxels, not of 64.
struct DtiScale { double ics[7]; };            // 1 / column scale of the design matrix
constexpr int kDtiNormLd = 37;                 // 28 + 7 sums per voxel, odd row stride
constexpr int kLmTrips = 64;                    // trip cap of the NLLS loop (10 on average, 32 at most in a numpy emulation)

__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

__device__ __forceinline__ double lanes_sum(double x)
{
#pragma unroll
    for (int m = 1; m < kDtiLanes; m <<= 1) x += __shfl_xor(x, m);
    return x;
}

// (A + lam diag A) x = b for the symmetric positive definite A (lower triangle, packed by rows), in place: A becomes its
// Cholesky factor (1 / pivot on the diagonal), b becomes x.  false when a pivot is not positive.
__device__ __forceinline__ bool chol_solve7(double (&A)[28], double (&b)[7], double lam)
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double d = fma(A[tri(j, j)], lam, A[tri(j, j)]);
#pragma unroll
        for (int k = 0; k < j; k++) d = fma(-A[tri(j, k)], A[tri(j, k)], d);
        const bool pos = d > 1e-280 && d < 1e280;
        ok = ok && pos;
        const double inv = fast_rsqrt(pos ? d : 1.0);
        A[tri(j, j)] = inv;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double t = A[tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) t = fma(-A[tri(i, k)], A[tri(j, k)], t);
            A[tri(i, j)] = t * inv;
        }
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double t = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) t = fma(-A[tri(i, k)], b[k], t);
        b[i] = t * A[tri(i, i)];
    }
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double t = b[i];
#pragma unroll
        for (int k = i + 1; k < 7; k++) t = fma(-A[tri(k, i)], b[k], t);
        b[i] = t * A[tri(i, i)];
    }
    return ok;
}

// one lane's share (volumes q, q + 8, ..) of the weighted normal equations, summed over the voxel's lanes:
// G = X^T W^2 X, g = X^T W^2 log s with W = exp(X p)
// REFIT (step 4 of RESTORE): the row holds s, not log s, and the lane's volume q + 8 j has the sample weight 0 where bit j of
// `skip` is set and 1 elsewhere
template <bool REFIT = false>
__device__ __forceinline__ void wls_pass(const double *__restrict__ xl, const double *__restrict__ yr, int nS, int q,
                                         const double (&p)[7], double (&G)[28], double (&g)[7], unsigned long long skip = 0)
{
#pragma unroll
    for (int k = 0; k < 28; k++) G[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 7; k++) g[k] = 0.0;
#pragma unroll 1
    for (int v = q; v < nS; v += kDtiLanes) {
        if constexpr (REFIT) {
            const bool out = skip & 1;
            skip >>= 1;
            if (out) continue;
        }
        double x[7], t = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) { x[k] = xl[v * 7 + k]; t = fma(x[k], p[k], t); }
        const double w2 = exp(2.0 * t), ly = REFIT ? log(yr[v]) : yr[v];
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const double wx = w2 * x[j];
            g[j] = fma(wx, ly, g[j]);
#pragma unroll
            for (int k = 0; k <= j; k++) G[tri(j, k)] = fma(wx, x[k], G[tri(j, k)]);
        }
    }
    // (in chunks: left to itself the scheduler keeps the sources and results of all 35 butterflies live at once)
#pragma unroll
    for (int k0 = 0; k0 < 28; k0 += 7) {
#pragma unroll
        for (int k = k0; k < k0 + 7; k++) G[k] = lanes_sum(G[k]);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < 7; k++) g[k] = lanes_sum(g[k]);
    __builtin_amdgcn_sched_barrier(0);
}

// the same for the non-linear cost at p: e = exp(X p), r = s - e, c = sum r^2, G = J^T J, g = J^T r with J = e (.) X
// REFIT: the sample weights of `skip`, as in wls_pass
template <bool REFIT = false>
__device__ __forceinline__ void nlls_pass(const double *__restrict__ xl, const double *__restrict__ sr, int nS, int q,
                                          const double (&p)[7], double &c, double (&G)[28], double (&g)[7], unsigned long long skip = 0)
{
    c = 0.0;
#pragma unroll
    for (int k = 0; k < 28; k++) G[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 7; k++) g[k] = 0.0;
#pragma unroll 1
    for (int v = q; v < nS; v += kDtiLanes) {
        if constexpr (REFIT) {
            const bool out = skip & 1;
            skip >>= 1;
            if (out) continue;
        }
        double x[7], t = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) { x[k] = xl[v * 7 + k]; t = fma(x[k], p[k], t); }
        const double e = exp(t), r = sr[v] - e;
        c = fma(r, r, c);
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const double ex = e * x[j];
            g[j] = fma(ex, r, g[j]);
#pragma unroll
            for (int k = 0; k <= j; k++) G[tri(j, k)] = fma(ex, e * x[k], G[tri(j, k)]);
        }
    }
    c = lanes_sum(c);
    // (in chunks: left to itself the scheduler keeps the sources and results of all 35 butterflies live at once)
#pragma unroll
    for (int k0 = 0; k0 < 28; k0 += 7) {
#pragma unroll
        for (int k = k0; k < k0 + 7; k++) G[k] = lanes_sum(G[k]);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < 7; k++) g[k] = lanes_sum(g[k]);
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ int wave_sum(int x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m);
    return x;
}

// Levenberg-Marquardt on sum (s_i - exp(X_i p))^2 from p, for the voxels with `run` set (the same on the 8 lanes of a voxel); the
// loop is uniform over the wavefront.  sr: the voxel's signal row, gv: its kDtiNormLd doubles of LDS, ss = sum s_i^2.  Returns
// whether the voxel failed (a non-finite cost, the trip cap, lam > 1e12): p is then the starting point again.  trips / wtrips grow
// by the voxel's trips and by those its wavefront ran.
template <bool REFIT>
__device__ __forceinline__ bool nlls_fit(const double *__restrict__ xl, const double *__restrict__ sr, double *__restrict__ gv, int nS, int q,
                                         unsigned long long skip, double ss, bool run, double (&p)[7], int &trips, int &wtrips)
{
    // normal equations of the accepted point: parked in LDS between trips (every lane of the voxel writes the same bits
    // and reads its own back, so no ordering between lanes is needed); registers hold one set of 35 sums at a time
    double c, p0[7];
#pragma unroll
    for (int k = 0; k < 7; k++) p0[k] = p[k];
    {
        double G[28], g[7];
        nlls_pass<REFIT>(xl, sr, nS, q, p, c, G, g, skip);
        if (run) {
#pragma unroll
            for (int k = 0; k < 28; k++) gv[k] = G[k];
#pragma unroll
            for (int k = 0; k < 7; k++) gv[28 + k] = g[k];
        }
    }
    bool failed = run && !(c < 1e300);
    bool active = run && !failed;
    double lam = 1e-3;
    const double floor_c = 1e-30 * ss;         // an exact fit (7 volumes) ends at rounding noise of the signal, not at zero
#pragma unroll 1
    for (int trip = 0; trip < kLmTrips; trip++) {
        if (!__any(active)) break;             // the loop is uniform over the wavefront: the shuffles see every lane
        wtrips++;
        double pt[7];
        bool ok;
        {
            double G[28], g[7];
#pragma unroll
            for (int k = 0; k < 28; k++) G[k] = gv[k];
#pragma unroll
            for (int k = 0; k < 7; k++) g[k] = gv[28 + k];
            ok = chol_solve7(G, g, lam);
#pragma unroll
            for (int k = 0; k < 7; k++) pt[k] = ok ? p[k] + g[k] : p[k];
        }
        double ct, Gt[28], gt[7];
        nlls_pass<REFIT>(xl, sr, nS, q, pt, ct, Gt, gt, skip);
        if (active) {
            trips++;
            const bool acc = ok && ct <= c;    // (false for a non-finite trial cost)
            const bool flat = ok && fabs(c - ct) <= fma(1e-15, c, floor_c);
            if (acc) {
#pragma unroll
                for (int k = 0; k < 7; k++) { p[k] = pt[k]; gv[28 + k] = gt[k]; }
#pragma unroll
                for (int k = 0; k < 28; k++) gv[k] = Gt[k];
                c = ct;
                lam = fmax(lam * 0.1, 1e-12);
            } else {
                lam *= 10.0;
            }
            if (flat && trip >= 2) active = false;                  // converged: the cost has stopped moving in fp64
            else if (lam > 1e12) { active = false; failed = true; }
        }
    }
    failed = failed || active;                 // trip cap
#pragma unroll
    for (int k = 0; k < 7; k++) p[k] = failed ? p0[k] : p[k];
    return failed;
}

// ---------------------------------------------------------------------------------------------------------------------------
// RESTORE (include/amico_amd.h: steps 1-5).  Step 1 is the NLLS fit above.  What follows runs only while a voxel of the wavefront
// has a sample beyond 3 sigma; the other voxels idle.  A voxel's residuals live in a second LDS row beside its signals, each lane
// writing its own volumes and all eight reading the whole row (same wavefront: the fence orders the two); the outlier set is one
// bit per volume in a register of the lane that owns the volume (64 volumes per lane: schemes of up to 512).
constexpr int kGmTrips = 1024;                  // trip cap of step 3 (62 on average, 440 at most in a numpy emulation on 33 .. 288 volumes)
constexpr int kDtiStats = 8;                    // counters of a call (amx_dti in amx_host.hpp)

__device__ __forceinline__ double lanes_max(double x)
{
#pragma unroll
    for (int m = 1; m < kDtiLanes; m <<= 1) x = fmax(x, __shfl_xor(x, m));
    return x;
}

__device__ __forceinline__ int lanes_sum(int x)
{
#pragma unroll
    for (int m = 1; m < kDtiLanes; m <<= 1) x += __shfl_xor(x, m);
    return x;
}

__device__ __forceinline__ void row_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// r = s - exp(X p) at the lane's volumes: the bits of those beyond thr (a NaN residual is none); returns their count in the voxel
__device__ __forceinline__ int restore_verdict(const double *__restrict__ xl, const double *__restrict__ sr, int nS, int q,
                                               const double (&p)[7], double thr, unsigned long long &skip)
{
    skip = 0;
    unsigned long long bit = 1;
#pragma unroll 1
    for (int v = q; v < nS; v += kDtiLanes, bit <<= 1) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) t = fma(xl[v * 7 + k], p[k], t);
        if (fabs(sr[v] - exp(t)) > thr) skip |= bit;
    }
    return lanes_sum((int)__popcll(skip));
}

// numpy's median of the row (DEV: of |row - centre|) by rank counting: each lane ranks its own volumes against the whole row; the
// value with `less <= k < less + equal` is the k-th smallest.  The mean of the two middle values for an even count.
template <bool DEV>
__device__ __forceinline__ double row_median(const double *rr, int nS, int q, double centre)
{
    const int k2 = nS >> 1, k1 = (nS & 1) ? k2 : k2 - 1;
    double lo = -INFINITY, hi = -INFINITY;
#pragma unroll 1
    for (int v = q; v < nS; v += kDtiLanes) {
        const double a = DEV ? fabs(rr[v] - centre) : rr[v];
        int less = 0, same = 0;
#pragma unroll 4
        for (int j = 0; j < nS; j++) {
            const double b = DEV ? fabs(rr[j] - centre) : rr[j];
            less += b < a ? 1 : 0;
            same += b == a ? 1 : 0;
        }
        if (less <= k1 && k1 < less + same) lo = a;
        if (less <= k2 && k2 < less + same) hi = a;
    }
    return 0.5 * (lanes_max(lo) + lanes_max(hi));
}

// the Geman-McClure weight of a residual, w = wn / (r^2 + C^2) with wn = 1 / mean(1 / (r^2 + C^2))
__device__ __forceinline__ double gm_weight(double r, double C2, double wn) { return wn / fma(r, r, C2); }

// nlls_pass with the frozen weights of the residual row rr (taken at the point the weights belong to):
// c = sum w r^2, G = J^T W J, g = J^T W r at p
__device__ __forceinline__ void gm_pass(const double *__restrict__ xl, const double *__restrict__ sr, const double *rr,
                                        int nS, int q, const double (&p)[7], double C2, double wn, double &c, double (&G)[28],
                                        double (&g)[7])
{
    c = 0.0;
#pragma unroll
    for (int k = 0; k < 28; k++) G[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 7; k++) g[k] = 0.0;
#pragma unroll 1
    for (int v = q; v < nS; v += kDtiLanes) {
        double x[7], t = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) { x[k] = xl[v * 7 + k]; t = fma(x[k], p[k], t); }
        const double e = exp(t), r = sr[v] - e, w = gm_weight(rr[v], C2, wn), we = w * e;
        c = fma(w * r, r, c);
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const double ex = we * x[j];
            g[j] = fma(ex, r, g[j]);
#pragma unroll
            for (int k = 0; k <= j; k++) G[tri(j, k)] = fma(ex, e * x[k], G[tri(j, k)]);
        }
    }
    c = lanes_sum(c);
#pragma unroll
    for (int k0 = 0; k0 < 28; k0 += 7) {
#pragma unroll
        for (int k = k0; k < k0 + 7; k++) G[k] = lanes_sum(G[k]);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < 7; k++) g[k] = lanes_sum(g[k]);
    __builtin_amdgcn_sched_barrier(0);
}

// Step 3 for the voxels with `need` set: p1 -> p2.  Returns whether the voxel reached the trip cap or gave up.
__device__ __forceinline__ bool restore_reweighted(const double *__restrict__ xl, const double *__restrict__ sr, double *rr,
                                                   int nS, int q, double sigma, bool need, double (&p)[7], int &trips, int &wtrips)
{
    bool active = need, gave_up = false;
    double lam = 1e-3;
#pragma unroll 1
    for (int trip = 0; trip < kGmTrips; trip++) {
        if (!__any(active)) break;
        wtrips++;
#pragma unroll 1
        for (int v = q; v < nS; v += kDtiLanes) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 7; k++) t = fma(xl[v * 7 + k], p[k], t);
            const double r = sr[v] - exp(t);
            if (active) rr[v] = r;
        }
        row_fence();
        const double med = row_median<false>(rr, nS, q, 0.0);
        const double mad = row_median<true>(rr, nS, q, med);
        const double C = fmax(1.4826 * mad, 1e-6 * sigma), C2 = C * C;
        double sw = 0.0;
#pragma unroll 1
        for (int v = q; v < nS; v += kDtiLanes) sw += gm_weight(rr[v], C2, 1.0);
        const double wn = (double)nS / lanes_sum(sw);
        double c, d[7], pt[7];
        bool ok;
        {
            double G[28];
            gm_pass(xl, sr, rr, nS, q, p, C2, wn, c, G, d);
            ok = chol_solve7(G, d, lam);
#pragma unroll
            for (int k = 0; k < 7; k++) pt[k] = ok ? p[k] + d[k] : p[k];
        }
        // the trial: the frozen-weight cost at pt and the largest move of a sample's log-signal
        double ct = 0.0, dmax = 0.0;
#pragma unroll 1
        for (int v = q; v < nS; v += kDtiLanes) {
            double t = 0.0, u = 0.0;
#pragma unroll
            for (int k = 0; k < 7; k++) { const double x = xl[v * 7 + k]; t = fma(x, pt[k], t); u = fma(x, d[k], u); }
            const double r = sr[v] - exp(t);
            ct = fma(gm_weight(rr[v], C2, wn) * r, r, ct);
            dmax = fmax(dmax, fabs(u));
        }
        ct = lanes_sum(ct);
        dmax = lanes_max(dmax);
        row_fence();                           // the row is read to the end before the next trip rewrites it
        if (active) {
            trips++;
            if (ok && ct <= c) {               // (false for a non-finite trial cost)
#pragma unroll
                for (int k = 0; k < 7; k++) p[k] = pt[k];
                lam = fmax(lam * 0.1, 1e-12);
                if (dmax <= 1e-10) active = false;
            } else {
                lam *= 10.0;
                if (lam > 1e12) { active = false; gave_up = true; }
            }
        }
    }
    return gave_up || active;
}

enum { kDtiWls = AMX_DTI_WLS, kDtiNlls = AMX_DTI_NLLS, kDtiRestore = AMX_DTI_RESTORE };

// y f64|f32[n][nS] -> dirs f64[n][3].  wt7 f64[nS][7]: pinv(X)^T with row k scaled by the column scale of X; xs f64[nS][7]: X
// with its columns scaled to unit max-abs.  stats (NLLS, RESTORE): [0] voxels that kept their starting parameters, [1] trips of the
// voxels, [2] trips their wavefronts made for them (a voxel waits for the slowest of the 8 in its wavefront); RESTORE: [4] voxels
// that entered step 3, [5] refitted in step 4, [6] at step 3's cap or give-up, [7] with fewer than 7 inliers; outliers i32[n] or null.
// MAPS: dti_store's.
template <typename YT, int METHOD, bool MAPS>
__global__ __launch_bounds__(kDtiThreads, METHOD != kDtiWls ? 1 : 2) void k_dti_dirs_w(const YT *__restrict__ y, const double *__restrict__ wt7,
                                                                        const double *__restrict__ xs, DtiScale sc,
                                                                        int nS, int ldl, int tv, long long n, double min_signal,
                                                                        double *__restrict__ dirs, unsigned long long *__restrict__ stats,
                                                                        double min_diffusivity, double *__restrict__ evals,
                                                                        double *__restrict__ scalars, double sigma,
                                                                        int *__restrict__ outliers)
{
    constexpr bool NLLS = METHOD != kDtiWls;           // the non-linear fit runs (RESTORE: as its step 1)
    extern __shared__ double sm[];
    double *wl = sm;                                   // nS * 7
    double *xl = sm + nS * 7;                          // nS * 7 (odd row stride)
    double *yl = sm + ((nS * 14 + 1) & ~1);            // tv * ldl
    double *dl = yl + tv * ldl;                        // kDtiBatch * tv * 7 (6 tensor entries, odd stride)
    double *gl = dl + kDtiBatch * tv * 7;              // NLLS: tv * kDtiNormLd (normal equations of each voxel's accepted point)
    double *rl = gl + tv * kDtiNormLd;                 // RESTORE: tv * ldl (residual rows)
    const int tid = threadIdx.x;
    for (int i = tid; i < nS * 7; i += kDtiThreads) { wl[i] = wt7[i]; xl[i] = xs[i]; }
    const long long n_tiles = (n + tv - 1) / tv;
    const int step = 2 * kDtiThreads;
    const int step_vol = step % nS, step_adr = (step / nS) * ldl + step_vol;
    const int vox0 = (2 * tid) / nS, vol0 = 2 * tid - vox0 * nS, adr0 = vox0 * ldl + vol0;
    const int eslot = tid / tv, evox = tid - eslot * tv;      // tensor this thread diagonalises in a batch
    double2 pre[kDtiPre];
#pragma unroll
    for (int i = 0; i < kDtiPre; i++) pre[i] = make_double2(1.0, 1.0);
    long long tile = blockIdx.x;
    if (tile < n_tiles) {
        const long long v0 = tile * tv;
        dti_prefetch(pre, y + v0 * nS, (int)((n - v0) < tv ? (n - v0) : tv) * nS, tid);
    }
    long long batch_tile = tile;
    int slot = 0;
    for (; tile < n_tiles; tile += gridDim.x) {
        const long long v0 = tile * tv;
        const int nv = (int)((n - v0) < tv ? (n - v0) : tv);
        const int cnt = nv * nS;
#pragma unroll
        for (int i = 0; i < kDtiPre; i++) {            // (four chains at a time: the registers belong to the normal equations here)
            pre[i].x = fast_log(fmax(pre[i].x, min_signal));
            pre[i].y = fast_log(fmax(pre[i].y, min_signal));
            if (i & 1) __builtin_amdgcn_sched_barrier(0);
        }
        int vol = vol0, adr = adr0;
#pragma unroll
        for (int i = 0; i < kDtiPre; i++) {
            const int e = 2 * (tid + i * kDtiThreads);
            if (e < cnt) yl[adr] = pre[i].x;
            if (e + 1 < cnt) yl[vol + 1 == nS ? adr + 1 + ldl - nS : adr + 1] = pre[i].y;
            vol += step_vol; adr += step_adr;
            if (vol >= nS) { vol -= nS; adr += ldl - nS; }
        }
        __syncthreads();                               // log-signals of this tile are in LDS
        const long long nt = tile + gridDim.x;
        if (nt < n_tiles) {
            const long long w0 = nt * tv;
            dti_prefetch(pre, y + w0 * nS, (int)((n - w0) < tv ? (n - w0) : tv) * nS, tid);
        }
        const int vox = tid / kDtiLanes, q = tid % kDtiLanes;
        const bool live = vox < nv;
        double *yr = yl + (live ? vox : 0) * ldl;      // (lanes without a voxel go through the motions on row 0 and store nothing)
        // pass 1: all seven OLS parameters (ln S0 is needed for the weights), in the scaled parametrisation
        double p[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int v = q; v < nS; v += kDtiLanes) {
            const double ly = yr[v];
            const double *w = wl + v * 7;
#pragma unroll
            for (int k = 0; k < 7; k++) p[k] = fma(w[k], ly, p[k]);
        }
#pragma unroll
        for (int k = 0; k < 7; k++) p[k] = lanes_sum(p[k]);
        // pass 2: weighted normal equations; a voxel whose system is not positive definite keeps the OLS parameters
        {
            double G[28], g[7];
            wls_pass(xl, yr, nS, q, p, G, g);
            bool ok = chol_solve7(G, g, 0.0);
#pragma unroll
            for (int k = 0; k < 7; k++) ok = ok && fabs(g[k]) < 1e300;
#pragma unroll
            for (int k = 0; k < 7; k++) p[k] = ok ? g[k] : p[k];
        }
        if constexpr (NLLS) {
            // the row becomes the signal itself (each lane its own entries; nobody else reads them before the next barrier)
            double ss = 0.0;
            for (int v = q; v < nS; v += kDtiLanes) {
                const double sv = exp(yr[v]);
                if (live) yr[v] = sv;
                ss = fma(sv, sv, ss);
            }
            ss = lanes_sum(ss);
            double *gv = gl + (live ? vox : 0) * kDtiNormLd;
            int trips = 0, wtrips = 0;
            bool failed = nlls_fit<false>(xl, yr, gv, nS, q, 0ull, ss, live, p, trips, wtrips);
            if constexpr (METHOD == kDtiRestore) {
                const double thr = 3.0 * sigma;
                unsigned long long skip;
                int n_out = restore_verdict(xl, yr, nS, q, p, thr, skip);
                const bool need = live && n_out > 0;
                bool capped = false, refit = false, few = false;
                if (__any(need)) {
                    // (lanes without a voxel go through the motions on residual row 0, as on signal row 0.  Those of other wavefronts
                    //  than voxel 0's read it while it is rewritten: what they compute is never stored and every loop is bounded)
                    capped = restore_reweighted(xl, yr, rl + (live ? vox : 0) * ldl, nS, q, sigma, need, p, trips, wtrips);
                    n_out = restore_verdict(xl, yr, nS, q, p, thr, skip);
                    few = need && n_out > 0 && nS - n_out < 7;
                    refit = need && n_out > 0 && !few;
                    if (__any(refit)) {
                        // OLS (the weights of wls_pass at p = 0 are exp(0) = 1), WLS and NLLS over the samples outside O
                        double pr[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                        bool ok0;
                        {
                            double G[28], g[7];
                            wls_pass<true>(xl, yr, nS, q, pr, G, g, skip);
                            ok0 = chol_solve7(G, g, 0.0);
#pragma unroll
                            for (int k = 0; k < 7; k++) ok0 = ok0 && fabs(g[k]) < 1e300;
#pragma unroll
                            for (int k = 0; k < 7; k++) pr[k] = ok0 ? g[k] : 0.0;
                            wls_pass<true>(xl, yr, nS, q, pr, G, g, skip);
                            bool ok = chol_solve7(G, g, 0.0);
#pragma unroll
                            for (int k = 0; k < 7; k++) ok = ok && fabs(g[k]) < 1e300;
#pragma unroll
                            for (int k = 0; k < 7; k++) pr[k] = ok ? g[k] : pr[k];
                        }
                        const bool bad = nlls_fit<true>(xl, yr, gv, nS, q, skip, ss, refit && ok0, pr, trips, wtrips);
                        if (refit) {
#pragma unroll
                            for (int k = 0; k < 7; k++) p[k] = ok0 ? pr[k] : p[k];
                            failed = failed || bad || !ok0;
                        }
                    }
                }
                if (!need) n_out = 0;
                const bool head = live && q == 0;
                if (head && outliers) outliers[v0 + vox] = n_out;
                const int s3 = wave_sum(head && need ? 1 : 0), s4 = wave_sum(head && refit ? 1 : 0),
                          sc3 = wave_sum(head && capped ? 1 : 0), sf = wave_sum(head && few ? 1 : 0);
                if ((tid & 63) == 0 && s3) {
                    atomicAdd(stats + 4, (unsigned long long)s3);
                    if (s4) atomicAdd(stats + 5, (unsigned long long)s4);
                    if (sc3) atomicAdd(stats + 6, (unsigned long long)sc3);
                    if (sf) atomicAdd(stats + 7, (unsigned long long)sf);
                }
            }
            const bool head = live && q == 0;
            const int nf = wave_sum(head && failed ? 1 : 0), vt = wave_sum(head ? trips : 0), wt = wave_sum(head ? wtrips : 0);
            if ((tid & 63) == 0) {
                if (nf) atomicAdd(stats, (unsigned long long)nf);
                atomicAdd(stats + 1, (unsigned long long)vt);
                atomicAdd(stats + 2, (unsigned long long)wt);
            }
        }
        if (q == 0 && live) {
#pragma unroll
            for (int k = 0; k < 6; k++) dl[(slot * tv + vox) * 7 + k] = p[k] * sc.ics[k];
        }
        slot++;
        __syncthreads();                               // tensors in LDS; the signal rows may be overwritten
        if (slot == kDtiBatch || nt >= n_tiles) {
            if (eslot < slot) {
                const long long e0 = (batch_tile + (long long)eslot * gridDim.x) * tv;
                if (e0 + evox < n) {
                    double d[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) d[k] = dl[(eslot * tv + evox) * 7 + k];
                    dti_store<MAPS>(d, e0 + evox, dirs, min_diffusivity, evals, scalars);
                }
            }
            slot = 0;
            batch_tile = nt;
        }
    }
}

}  // namespace amx

static int dti_create(amx_ctx *ctx, const double *design, const double *inv_design, int nS, double min_signal, int method, double sigma,
                      amx_dti **out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!inv_design || !out || nS < 7 || nS > 2048) return amx_bad(ctx, "amx_dti_create: need inv_design f64[7][nS], 7 <= nS <= 2048");
    if (!(min_signal > 0.0)) return amx_bad(ctx, "amx_dti_create: min_signal must be positive");
    if (method != AMX_DTI_OLS && !design) return amx_bad(ctx, "amx_dti_create_method: WLS, NLLS and RESTORE need the design matrix f64[nS][7]");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> wt((size_t)nS * 6);
    for (int v = 0; v < nS; v++)
        for (int k = 0; k < 6; k++) wt[(size_t)v * 6 + k] = inv_design[(size_t)k * nS + v];
    amx_dti *h = new amx_dti;
    h->ctx = ctx; h->nS = nS; h->min_signal = min_signal; h->method = method; h->sigma = sigma;
    hipError_t e = hipMalloc((void **)&h->wt, wt.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(h->wt, wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && method != AMX_DTI_OLS) {
        // columns of the design matrix scaled to unit max-abs: the fit runs in p * scale, the kernel undoes it on the tensor
        std::vector<double> tab((size_t)nS * 14);                   // [nS][7] scaled pinv^T, then [nS][7] scaled design
        for (int k = 0; k < 7; k++) {
            double cs = 0.0;
            for (int v = 0; v < nS; v++) cs = std::fmax(cs, std::fabs(design[(size_t)v * 7 + k]));
            if (!(cs > 0.0) || !std::isfinite(cs)) cs = 1.0;
            h->ics[k] = 1.0 / cs;
            for (int v = 0; v < nS; v++) {
                tab[(size_t)v * 7 + k] = inv_design[(size_t)k * nS + v] * cs;
                tab[(size_t)(nS + v) * 7 + k] = design[(size_t)v * 7 + k] / cs;
            }
        }
        e = hipMalloc((void **)&h->wt7, tab.size() * sizeof(double) + kDtiStats * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemcpy(h->wt7, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            h->xs = h->wt7 + (size_t)nS * 7;
            h->stats = reinterpret_cast<unsigned long long *>(h->wt7 + (size_t)nS * 14);
            e = hipMemset(h->stats, 0, kDtiStats * sizeof(unsigned long long));
        }
    }
    if (e != hipSuccess) {
        if (h->wt) (void)hipFree(h->wt);
        if (h->wt7) (void)hipFree(h->wt7);
        delete h;
        ctx->err = std::string("amx_dti_create: ") + hipGetErrorString(e);
        return AMX_E_HIP;
    }
    *out = h;
    return AMX_OK;
}

extern "C" {

int amx_dti_create_method(amx_ctx *ctx, const double *design, const double *inv_design, int nS, double min_signal, int method,
                          amx_dti **out)
{
    if (!ctx) return AMX_E_BADARG;
    if (method == AMX_DTI_RESTORE) return amx_bad(ctx, "amx_dti_create_method: RESTORE needs sigma (amx_dti_create_robust)");
    if (method != AMX_DTI_OLS && method != AMX_DTI_WLS && method != AMX_DTI_NLLS)
        return amx_bad(ctx, "amx_dti_create_method: method must be AMX_DTI_OLS, AMX_DTI_WLS or AMX_DTI_NLLS");
    return dti_create(ctx, design, inv_design, nS, min_signal, method, 0.0, out);
}

int amx_dti_create_robust(amx_ctx *ctx, const double *design, const double *inv_design, int nS, double min_signal, double sigma,
                          amx_dti **out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return amx_bad(ctx, "amx_dti_create_robust: sigma must be a finite number > 0");
    return dti_create(ctx, design, inv_design, nS, min_signal, AMX_DTI_RESTORE, sigma, out);
}

int amx_dti_create(amx_ctx *ctx, const double *inv_design, int nS, double min_signal, amx_dti **out)
{
    return amx_dti_create_method(ctx, nullptr, inv_design, nS, min_signal, AMX_DTI_OLS, out);
}

void amx_dti_destroy(amx_dti *h)
{
    if (!h) return;
    if (h->ctx) (void)hipSetDevice(h->ctx->device);
    if (h->wt) (void)hipFree(h->wt);
    if (h->wt7) (void)hipFree(h->wt7);
    delete h;
}

static int dti_read_stats(amx_ctx *ctx, const amx_dti *h, unsigned long long (&st)[kDtiStats])
{
    if (!ctx) return AMX_E_BADARG;
    if (!h || h->ctx != ctx) return amx_bad(ctx, "amx_dti_last_stats: not an estimator of this ctx");
    for (int k = 0; k < kDtiStats; k++) st[k] = 0;
    if (h->method != AMX_DTI_NLLS && h->method != AMX_DTI_RESTORE) return AMX_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(h->last_stream));
    HIPCHK(ctx, hipMemcpy(st, h->stats, sizeof st, hipMemcpyDeviceToHost));
    return AMX_OK;
}

int amx_dti_last_unconverged(amx_ctx *ctx, const amx_dti *h, int64_t *out)
{
    if (ctx && !out) return amx_bad(ctx, "amx_dti_last_unconverged: null output");
    unsigned long long st[kDtiStats];
    const int rc = dti_read_stats(ctx, h, st);
    if (rc == AMX_OK) *out = (int64_t)st[0];
    return rc;
}

int amx_dti_last_trips(amx_ctx *ctx, const amx_dti *h, int64_t *out_voxel_trips, int64_t *out_wavefront_trips)
{
    if (ctx && (!out_voxel_trips || !out_wavefront_trips)) return amx_bad(ctx, "amx_dti_last_trips: null output");
    unsigned long long st[kDtiStats];
    const int rc = dti_read_stats(ctx, h, st);
    if (rc == AMX_OK) { *out_voxel_trips = (int64_t)st[1]; *out_wavefront_trips = (int64_t)st[2]; }
    return rc;
}

int amx_dti_last_robust(amx_ctx *ctx, const amx_dti *h, int64_t out[4])
{
    if (ctx && !out) return amx_bad(ctx, "amx_dti_last_robust: null output");
    unsigned long long st[kDtiStats];
    const int rc = dti_read_stats(ctx, h, st);
    if (rc == AMX_OK)
        for (int k = 0; k < 4; k++) out[k] = (int64_t)st[4 + k];
    return rc;
}

}  // extern "C"

// what amx_dti_fit* adds to amx_dti_directions*, and amx_dti_fit_robust* to those
struct DtiMapsOut { double min_diffusivity; double *evals, *scalars; int32_t *outliers = nullptr; };

template <typename YT, int METHOD, bool MAPS>
static int dti_directions_w_dev(amx_ctx *ctx, const amx_dti *h, const YT *d_y, int64_t n_vox, double *d_dirs, hipStream_t s,
                                const DtiMapsOut &mo)
{
    const int nS = h->nS;
    int ldl = (nS + 3) & ~3;
    if (((ldl >> 2) & 1) == 0) ldl += 4;
    constexpr bool NLLS = METHOD != kDtiWls, RESTORE = METHOD == kDtiRestore;
    int tv = (kDtiPre * 2 * kDtiThreads) / nS;
    tv = tv > kDtiVox ? kDtiVox : (tv & ~1);
    // the two [nS][7] tables (scaled pinv, scaled design matrix), the signal rows, the tensors of a batch, NLLS' normal equations,
    // RESTORE's residual rows -- which make its tile the shorter one on long schemes
    const size_t fixed = (size_t)((nS * 14 + 1) & ~1);
    const size_t per_vox = (size_t)ldl * (RESTORE ? 2 : 1) + (size_t)kDtiBatch * 7 + (NLLS ? (size_t)kDtiNormLd : 0);
    if (RESTORE) {
        if (nS > 64 * kDtiLanes) return amx_bad(ctx, "amx_dti_directions: scheme too long for the LDS tile (RESTORE: at most 512 volumes)");
        const int fit = (int)((160 * 1024 / sizeof(double) - fixed) / per_vox) & ~1;
        tv = tv < fit ? tv : fit;
    }
    const size_t lds = (fixed + (size_t)tv * per_vox) * sizeof(double);
    if (tv < 2 || lds > 160 * 1024) return amx_bad(ctx, "amx_dti_directions: scheme too long for the LDS tile");
    static bool attr_set[64];
    if (!attr_set[ctx->device & 63]) {
        HIPCHK(ctx, hipFuncSetAttribute((const void *)k_dti_dirs_w<YT, METHOD, MAPS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set[ctx->device & 63] = true;
    }
    const long long n_tiles = (n_vox + tv - 1) / tv;
    const int per_cu = (int)((160 * 1024) / lds) < 1 ? 1 : (int)((160 * 1024) / lds);
    long long grid = 256LL * (per_cu > 8 ? 8 : per_cu);
    if (grid > n_tiles) grid = n_tiles;
    DtiScale sc;
    for (int k = 0; k < 7; k++) sc.ics[k] = h->ics[k];
    if (NLLS) HIPCHK(ctx, hipMemsetAsync(h->stats, 0, kDtiStats * sizeof(unsigned long long), s));
    h->last_stream = s;
    rec(ctx, 8, s);
    hipLaunchKernelGGL((k_dti_dirs_w<YT, METHOD, MAPS>), dim3((unsigned)grid), dim3(kDtiThreads), lds, s, d_y, h->wt7, h->xs, sc, nS, ldl, tv,
                       (long long)n_vox, h->min_signal, d_dirs, h->stats, mo.min_diffusivity, mo.evals, mo.scalars, h->sigma, mo.outliers);
    HIPCHK(ctx, hipGetLastError());
    rec(ctx, 9, s);
    return AMX_OK;
}

template <typename YT, bool MAPS>
static int dti_directions_dev(amx_ctx *ctx, const amx_dti *h, const YT *d_y, int64_t n_vox, double *d_dirs, void *hip_stream,
                              const DtiMapsOut &mo)
{
    if (!ctx) return AMX_E_BADARG;
    if (!h || h->ctx != ctx) return amx_bad(ctx, "amx_dti_directions: not an estimator of this ctx");
    if (n_vox < 0) return amx_bad(ctx, "amx_dti_directions: bad n_vox");
    if (MAPS && !(mo.min_diffusivity >= 0.0)) return amx_bad(ctx, "amx_dti_fit: min_diffusivity must be a number >= 0");
    if (n_vox == 0) return AMX_OK;
    if (!d_y || (!MAPS && !d_dirs)) return amx_bad(ctx, "amx_dti_directions: null buffer");
    if (sizeof(YT) == 8 && ((uintptr_t)d_y & 15) != 0) return amx_bad(ctx, "amx_dti_directions: y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (h->method == AMX_DTI_WLS) return dti_directions_w_dev<YT, kDtiWls, MAPS>(ctx, h, d_y, n_vox, d_dirs, s, mo);
    if (h->method == AMX_DTI_NLLS) return dti_directions_w_dev<YT, kDtiNlls, MAPS>(ctx, h, d_y, n_vox, d_dirs, s, mo);
    if (h->method == AMX_DTI_RESTORE) return dti_directions_w_dev<YT, kDtiRestore, MAPS>(ctx, h, d_y, n_vox, d_dirs, s, mo);
    const int nS = h->nS;
    int ldl = (nS + 3) & ~3;                  // row stride = 4 * odd doubles: the 16 quads of a wavefront read
    if (((ldl >> 2) & 1) == 0) ldl += 4;      // conflict-free LDS rows
    int tv = (kDtiPre * 2 * kDtiThreads) / nS;   // voxels per tile: what the prefetch registers hold, even, <= kDtiVox
    tv = tv > kDtiVox ? kDtiVox : (tv & ~1);
    const size_t lds = ((size_t)((nS * 6 + 1) & ~1) + (size_t)tv * ldl + (size_t)kDtiBatch * tv * 7) * sizeof(double);
    if (tv < 2 || lds > 160 * 1024) return amx_bad(ctx, "amx_dti_directions: scheme too long for the LDS tile");
    static bool attr_set[64];              // (per instantiation of this function template AND device: the attribute belongs to the pair)
    if (!attr_set[ctx->device & 63]) {
        HIPCHK(ctx, hipFuncSetAttribute((const void *)(k_dti_dirs<YT, MAPS>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set[ctx->device & 63] = true;
    }
    const long long n_tiles = (n_vox + tv - 1) / tv;
    const int per_cu = (int)((160 * 1024) / lds) < 1 ? 1 : (int)((160 * 1024) / lds);
    long long grid = 256LL * (per_cu > 8 ? 8 : per_cu);
    if (grid > n_tiles) grid = n_tiles;
    rec(ctx, 8, s);
    hipLaunchKernelGGL((k_dti_dirs<YT, MAPS>), dim3((unsigned)grid), dim3(kDtiThreads), lds, s, d_y, h->wt, nS, ldl, tv,
                       (long long)n_vox, h->min_signal, d_dirs, mo.min_diffusivity, mo.evals, mo.scalars);
    HIPCHK(ctx, hipGetLastError());
    rec(ctx, 9, s);
    return AMX_OK;
}

// amx_dti_directions* + the eigenvalues and the scalar maps.  With neither map output this IS amx_dti_directions*: the same checks,
// the same kernel, the same launch.
template <typename YT>
static int dti_fit_dev(amx_ctx *ctx, const amx_dti *h, const YT *d_y, int64_t n_vox, double min_diffusivity, double *d_dirs,
                       double *d_evals, double *d_scalars, void *hip_stream, int32_t *d_outliers = nullptr)
{
    // (the outlier counts alone: the MAPS variant, whose every output may be null -- the direction kernel stores its directions unasked)
    if (!d_evals && !d_scalars && (d_dirs || !d_outliers))
        return dti_directions_dev<YT, false>(ctx, h, d_y, n_vox, d_dirs, hip_stream, DtiMapsOut{0.0, nullptr, nullptr, d_outliers});
    return dti_directions_dev<YT, true>(ctx, h, d_y, n_vox, d_dirs, hip_stream, DtiMapsOut{min_diffusivity, d_evals, d_scalars, d_outliers});
}

// amx_dti_fit_robust*: a RESTORE estimator and nothing else
static int dti_robust_handle(amx_ctx *ctx, const amx_dti *h)
{
    if (!ctx) return AMX_E_BADARG;
    if (!h || h->ctx != ctx) return amx_bad(ctx, "amx_dti_directions: not an estimator of this ctx");
    if (h->method != AMX_DTI_RESTORE) return amx_bad(ctx, "amx_dti_fit_robust: not a RESTORE estimator (amx_dti_create_robust)");
    return AMX_OK;
}

// amx_dti_fit and amx_dti_fit_robust
static int dti_fit_host(amx_ctx *ctx, const amx_dti *h, const double *y, int64_t n_vox, double min_diffusivity, double *out_dirs,
                        double *out_evals, double *out_scalars, int32_t *out_outliers)
{
    if (n_vox == 0) return AMX_OK;
    if (n_vox < 0 || !y || (!out_dirs && !out_evals && !out_scalars && !out_outliers)) return amx_bad(ctx, "amx_dti_directions: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    // one device buffer behind y's: 3 + 3 + 4 doubles per voxel, and the outlier counts
    const size_t yb = (size_t)n_vox * h->nS * sizeof(double), vb = (size_t)n_vox * sizeof(double);
    if ((rc = amx_ensure(ctx, ctx->hy, yb))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hdirs, 10 * vb + (size_t)n_vox * sizeof(int32_t)))) return rc;
    double *dd = (double *)ctx->hdirs.p, *de = dd + 3 * n_vox, *ds = dd + 6 * n_vox;
    int32_t *dout = (int32_t *)(dd + 10 * n_vox);
    HIPCHK(ctx, hipMemcpyAsync(ctx->hy.p, y, yb, hipMemcpyHostToDevice, nullptr));
    if ((rc = dti_fit_dev<double>(ctx, h, (const double *)ctx->hy.p, n_vox, min_diffusivity, out_dirs ? dd : nullptr, out_evals ? de : nullptr,
                                  out_scalars ? ds : nullptr, nullptr, out_outliers ? dout : nullptr))) return rc;
    if (out_dirs) HIPCHK(ctx, hipMemcpyAsync(out_dirs, dd, 3 * vb, hipMemcpyDeviceToHost, nullptr));
    if (out_evals) HIPCHK(ctx, hipMemcpyAsync(out_evals, de, 3 * vb, hipMemcpyDeviceToHost, nullptr));
    if (out_scalars) HIPCHK(ctx, hipMemcpyAsync(out_scalars, ds, 4 * vb, hipMemcpyDeviceToHost, nullptr));
    if (out_outliers) HIPCHK(ctx, hipMemcpyAsync(out_outliers, dout, (size_t)n_vox * sizeof(int32_t), hipMemcpyDeviceToHost, nullptr));
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}

extern "C" {

int amx_dti_directions_device(amx_ctx *ctx, const amx_dti *h, const double *d_y, int64_t n_vox, double *d_dirs, void *hip_stream)
{
    return dti_directions_dev<double, false>(ctx, h, d_y, n_vox, d_dirs, hip_stream, DtiMapsOut{0.0, nullptr, nullptr});
}

int amx_dti_directions_device_f32(amx_ctx *ctx, const amx_dti *h, const float *d_y, int64_t n_vox, double *d_dirs, void *hip_stream)
{
    return dti_directions_dev<float, false>(ctx, h, d_y, n_vox, d_dirs, hip_stream, DtiMapsOut{0.0, nullptr, nullptr});
}

int amx_dti_directions(amx_ctx *ctx, const amx_dti *h, const double *y, int64_t n_vox, double *out_dirs)
{
    if (!ctx) return AMX_E_BADARG;
    if (!h || h->ctx != ctx) return amx_bad(ctx, "amx_dti_directions: not an estimator of this ctx");
    if (n_vox == 0) return AMX_OK;
    if (n_vox < 0 || !y || !out_dirs) return amx_bad(ctx, "amx_dti_directions: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t yb = (size_t)n_vox * h->nS * sizeof(double), db = (size_t)n_vox * 3 * sizeof(double);
    if ((rc = amx_ensure(ctx, ctx->hy, yb))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hdirs, db))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->hy.p, y, yb, hipMemcpyHostToDevice, nullptr));
    if ((rc = amx_dti_directions_device(ctx, h, (const double *)ctx->hy.p, n_vox, (double *)ctx->hdirs.p, nullptr))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_dirs, ctx->hdirs.p, db, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}

int amx_dti_fit_device(amx_ctx *ctx, const amx_dti *h, const double *d_y, int64_t n_vox, double min_diffusivity, double *d_dirs,
                       double *d_evals, double *d_scalars, void *hip_stream)
{
    return dti_fit_dev<double>(ctx, h, d_y, n_vox, min_diffusivity, d_dirs, d_evals, d_scalars, hip_stream);
}

int amx_dti_fit_device_f32(amx_ctx *ctx, const amx_dti *h, const float *d_y, int64_t n_vox, double min_diffusivity, double *d_dirs,
                           double *d_evals, double *d_scalars, void *hip_stream)
{
    return dti_fit_dev<float>(ctx, h, d_y, n_vox, min_diffusivity, d_dirs, d_evals, d_scalars, hip_stream);
}

int amx_dti_fit(amx_ctx *ctx, const amx_dti *h, const double *y, int64_t n_vox, double min_diffusivity, double *out_dirs,
                double *out_evals, double *out_scalars)
{
    if (!ctx) return AMX_E_BADARG;
    if (!h || h->ctx != ctx) return amx_bad(ctx, "amx_dti_directions: not an estimator of this ctx");
    return dti_fit_host(ctx, h, y, n_vox, min_diffusivity, out_dirs, out_evals, out_scalars, nullptr);
}

int amx_dti_fit_robust_device(amx_ctx *ctx, const amx_dti *h, const double *d_y, int64_t n_vox, double min_diffusivity, double *d_dirs,
                              double *d_evals, double *d_scalars, int32_t *d_outliers, void *hip_stream)
{
    const int rc = dti_robust_handle(ctx, h);
    return rc ? rc : dti_fit_dev<double>(ctx, h, d_y, n_vox, min_diffusivity, d_dirs, d_evals, d_scalars, hip_stream, d_outliers);
}

int amx_dti_fit_robust_device_f32(amx_ctx *ctx, const amx_dti *h, const float *d_y, int64_t n_vox, double min_diffusivity, double *d_dirs,
                                  double *d_evals, double *d_scalars, int32_t *d_outliers, void *hip_stream)
{
    const int rc = dti_robust_handle(ctx, h);
    return rc ? rc : dti_fit_dev<float>(ctx, h, d_y, n_vox, min_diffusivity, d_dirs, d_evals, d_scalars, hip_stream, d_outliers);
}

int amx_dti_fit_robust(amx_ctx *ctx, const amx_dti *h, const double *y, int64_t n_vox, double min_diffusivity, double *out_dirs,
                       double *out_evals, double *out_scalars, int32_t *out_outliers)
{
    const int rc = dti_robust_handle(ctx, h);
    return rc ? rc : dti_fit_host(ctx, h, y, n_vox, min_diffusivity, out_dirs, out_evals, out_scalars, out_outliers);
}

}  // extern "C"
