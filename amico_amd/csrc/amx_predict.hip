// amx_predict.hip -- the signal the fitted model predicts, from the dictionary and the coefficients a fit leaves (AMX_F_DEBUG_X):
//     y_est[i, s] = sum_j A_i[s, j] x_i[j]          what _compute_rmse / _compute_nrmse take the residual of (models.pyx:47-71)
// A_i = the tile of the voxel's orientation as it lies in HBM (lut->tiles, [ndirs][nS][ldA]; SANDI: the one dictionary), x_i = row i of
// the caller's coefficient buffer (x_stride / x_offset pick NODDI's debiased stage-3 row out of the [n][3][n_atoms] layout).
// ONE streaming kernel in two output forms, the shape of k_fw_corrected (amx_fw_corrected.hip): rows f64[n][nS], and the float32 volume
// [X][Y][Z][nS] with the b0 mean folded in and zeros outside the mask.  The lanes run along the FLATTENED (voxel, volume) index of a
// block of kPredVox voxels that are consecutive in the output, so the writes are whole lines whatever nS is.  Per workgroup and once:
// the block's rows, LUT indices and b0 means go to LDS, and every voxel's coefficient vector is COMPACTED there -- its non-zero
// (atom, value) pairs in ascending atom order; NODDI's optimum holds 5 .. 15 atoms of 145, so a sample costs nnz gathers from the tile
// instead of n_atoms.  A vector of more than kPredCap non-zeros is not truncated: its samples walk the dense vector in HBM.
// Arithmetic: fp64, atoms ascending, every product and every sum rounded on its own (no fused multiply-add); a coefficient that is
// exactly 0 is skipped (adding +-0 to the partial sum changes nothing), a NaN is not: it makes the row NaN.
#include "amx_host.hpp"

namespace amx {

constexpr int kPredVox = 64;       // voxels per workgroup
constexpr int kPredCap = 16;       // non-zero coefficients per voxel kept in LDS (more: dense walk)
constexpr int kPredLd = kPredCap + 1;

struct PredArgs {
    const void *tiles;             // T [ndirs][tile_stride]: rows of ldA atoms
    long long tile_stride;         // elements between two orientations
    int nS, ldA, n_atoms;
    const double *x;               // coefficients of row r: x[r * x_stride + x_offset + j]
    long long x_stride, x_offset;
    const int *lutidx;             // [n_vox]: orientation of row r, -1 = skipped by the fit; null: one dictionary (SANDI)
    long long n_items;             // rows form: voxels; volume form: voxels of the whole volume
    // volume form
    const int *rank;               // [d2][d1][d0] in the image's memory-axis order: row of the voxel, or -1
    long long d[3], c[3];          // extents of the memory axes and their strides in the C-ordered volume
    const float *mean_b0;          // [n_vox] or null (no rescaling)
    void *out;                     // rows: double [n_vox][nS]; volume: float [n_items][nS]
};

// acc = 0; for k: acc = acc + A[k] * x[k] -- one rounding per operation: hipcc contracts a * b + c into a fused multiply-add by default
// and its __dmul_rn / __dadd_rn are the plain operators, so contraction is switched off for these functions (as in amx_fw_corrected.hip)
template <typename T>
__device__ __forceinline__ double predict_listed(const T *__restrict__ row, const int *__restrict__ idx, const double *__restrict__ val, int nnz)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int k = 0; k < nnz; k++) { const double t = (double)row[idx[k]] * val[k]; acc = acc + t; }
    return acc;
}
template <typename T>
__device__ __forceinline__ double predict_dense(const T *__restrict__ row, const double *__restrict__ x, int n_atoms)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int j = 0; j < n_atoms; j++) {
        const double xv = x[j];
        if (xv == 0.0) continue;                                       // (a NaN is not 0)
        const double t = (double)row[j] * xv;
        acc = acc + t;
    }
    return acc;
}
__device__ __forceinline__ float predict_scaled(double v, double m)
{
#pragma clang fp contract(off)
    const double t = m * v;
    return (float)t;
}

template <typename T, bool VOLUME>
__global__ __launch_bounds__(256) void k_predict(const PredArgs a)
{
    __shared__ double vals[kPredVox * kPredLd];
    __shared__ double ms[kPredVox];
    __shared__ int idxs[kPredVox * kPredLd];
    __shared__ int rs[kPredVox], ls[kPredVox], nz[kPredVox];      // row (-1: not masked), orientation (-1: skipped), non-zeros (-1: beyond kPredCap)
    const int nS = a.nS, n_atoms = a.n_atoms;
    const long long v0 = (long long)blockIdx.x * kPredVox;
    const int nv = (int)(a.n_items - v0 < kPredVox ? a.n_items - v0 : kPredVox);
    if ((int)threadIdx.x < nv) {
        const int t = threadIdx.x;
        long long r = v0 + t;
        double m = 1.0;
        if (VOLUME) {
            // C-order position -> coordinates along the image's memory axes -> the plan's rank table
            const long long cpos = v0 + t;
            const long long i0 = (cpos / a.c[0]) % a.d[0], i1 = (cpos / a.c[1]) % a.d[1], i2 = (cpos / a.c[2]) % a.d[2];
            r = a.rank[(i2 * a.d[1] + i1) * a.d[0] + i0];
            if (r >= 0 && a.mean_b0) m = (double)a.mean_b0[r];
        }
        rs[t] = (int)r; ms[t] = m;
        ls[t] = r < 0 ? -1 : (a.lutidx ? a.lutidx[r] : 0);
    }
    __syncthreads();
    // compaction: one wavefront per voxel, 64 atoms a step; a lane's slot is the number of non-zeros below it (ascending atom order)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    for (int t = wave; t < nv; t += n_waves) {
        int count = 0;
        if (ls[t] >= 0) {
            const double *__restrict__ xr = a.x + (size_t)rs[t] * a.x_stride + a.x_offset;
            for (int j0 = 0; j0 < n_atoms; j0 += 64) {
                const int j = j0 + lane;
                const double xv = j < n_atoms ? xr[j] : 0.0;
                const bool on = !(xv == 0.0);
                const unsigned long long bits = __ballot(on);
                const int slot = count + __popcll(bits & ((1ull << lane) - 1ull));
                if (on && slot < kPredCap) { idxs[t * kPredLd + slot] = j; vals[t * kPredLd + slot] = xv; }
                count += __popcll(bits);
            }
        }
        if (lane == 0) nz[t] = count > kPredCap ? -1 : count;
    }
    __syncthreads();
    const unsigned total = (unsigned)nv * (unsigned)nS;
    const T *__restrict__ tiles = reinterpret_cast<const T *>(a.tiles);
    for (unsigned e = threadIdx.x; e < total; e += blockDim.x) {
        const unsigned t = e / (unsigned)nS;
        const int s = (int)(e - t * (unsigned)nS);
        const size_t o = (size_t)v0 * nS + e;
        const int r = rs[t], l = ls[t];
        double v = 0.0;                                                 // not masked, or skipped for its direction: zeros
        if (l >= 0) {
            const T *__restrict__ row = tiles + (size_t)l * a.tile_stride + (size_t)s * a.ldA;
            const int n = nz[t];
            v = n >= 0 ? predict_listed(row, idxs + t * kPredLd, vals + t * kPredLd, n)
                       : predict_dense(row, a.x + (size_t)r * a.x_stride + a.x_offset, n_atoms);
        }
        if (VOLUME) reinterpret_cast<float *>(a.out)[o] = l >= 0 ? predict_scaled(v, ms[t]) : 0.0f;
        else reinterpret_cast<double *>(a.out)[o] = v;
    }
}

}  // namespace amx

using namespace amx;

namespace {

// the checks the two forms share; the LUT index of every row comes from k_dir_to_lut (amx_plan.hip) into the context's own buffer
int pred_common(amx_ctx *ctx, const amx_lut *lut, const char *who, const double *d_x, int64_t x_stride, int64_t x_offset, const double *d_dirs,
                int64_t n_vox, PredArgs &a, hipStream_t s)
{
    const std::string w(who);
    if (!lut || lut->ctx != ctx || lut->model < 1 || lut->model > 4) return amx_bad(ctx, (w + ": not a dictionary of this ctx").c_str());
    const FitSpec &m = kFits[lut->model - 1];
    if (m.dirs && !d_dirs && n_vox > 0) return amx_bad(ctx, (w + ": a " + m.what + " dictionary needs the directions (d_dirs is NULL)").c_str());
    if (!m.dirs && d_dirs) return amx_bad(ctx, (w + ": a " + m.what + " dictionary takes no directions (d_dirs must be NULL)").c_str());
    if (x_offset < 0 || x_stride < x_offset + lut->n_atoms) return amx_bad(ctx, (w + ": x_stride is smaller than x_offset + n_atoms").c_str());
    if (n_vox > 0 && !d_x) return amx_bad(ctx, (w + ": null buffer").c_str());
    HIPCHK(ctx, hipSetDevice(ctx->device));
    a.tiles = lut->tiles; a.tile_stride = lut->tile_stride; a.nS = lut->nS; a.ldA = lut->ldA; a.n_atoms = lut->n_atoms;
    a.x = d_x; a.x_stride = x_stride; a.x_offset = x_offset;
    if (m.dirs && n_vox > 0) {
        int rc;
        if ((rc = amx_ensure(ctx, ctx->pred_idx, (size_t)n_vox * sizeof(int)))) return rc;
        if ((rc = enqueue_dir_to_lut(ctx, lut, d_dirs, n_vox, (int *)ctx->pred_idx.p, s))) return rc;
        a.lutidx = (const int *)ctx->pred_idx.p;
    }
    return AMX_OK;
}

template <bool VOLUME>
int pred_launch(amx_ctx *ctx, const amx_lut *lut, const PredArgs &a, hipStream_t s)
{
    const long long blocks = (a.n_items + kPredVox - 1) / kPredVox;
    if (lut->model == 3) hipLaunchKernelGGL((k_predict<double, VOLUME>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_predict<float, VOLUME>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

}  // namespace

extern "C" {

int amx_predict_device(amx_ctx *ctx, const amx_lut *lut, const double *d_x, int64_t x_stride, int64_t x_offset, const double *d_dirs,
                       int64_t n_vox, double *d_yest, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (n_vox < 0 || n_vox > INT_MAX / 4) return amx_bad(ctx, "amx_predict: bad n_vox");
    PredArgs a{};
    int rc;
    if ((rc = pred_common(ctx, lut, "amx_predict", d_x, x_stride, x_offset, d_dirs, n_vox, a, (hipStream_t)hip_stream))) return rc;
    if (n_vox == 0) return AMX_OK;
    if (!d_yest) return amx_bad(ctx, "amx_predict: null buffer");
    a.n_items = n_vox; a.out = d_yest;
    return pred_launch<false>(ctx, lut, a, (hipStream_t)hip_stream);
}

int amx_prep_predicted_device(amx_ctx *ctx, const amx_prep *p, const amx_lut *lut, const double *d_x, int64_t x_stride, int64_t x_offset,
                              const double *d_dirs, const float *d_mean_b0, float *d_volume, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_predicted: not a plan of this ctx");
    if (lut && lut->ctx == ctx && p->n_out != lut->nS) return amx_bad(ctx, "amx_prep_predicted: the plan prepares another number of volumes than the dictionary holds");
    if (!d_volume) return amx_bad(ctx, "amx_prep_predicted: null buffer");
    PredArgs a{};
    int rc;
    if ((rc = pred_common(ctx, lut, "amx_prep_predicted", d_x, x_stride, x_offset, d_dirs, p->n_vox, a, (hipStream_t)hip_stream))) return rc;
    if (p->n_total == 0) return AMX_OK;
    a.n_items = p->n_total; a.rank = p->rank; a.mean_b0 = d_mean_b0; a.out = d_volume;
    for (int k = 0; k < 3; k++) { a.d[k] = p->d[k]; a.c[k] = p->c[k]; }
    return pred_launch<true>(ctx, lut, a, (hipStream_t)hip_stream);
}

}  // extern "C"
