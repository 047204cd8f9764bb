// amx_fw_corrected.hip -- FreeWater's corrected DWI from the signals and the isotropic coefficients of the fit (AMX_F_FW_ISO):
//     y_corrected[i, j] = max(0, y[i, j] - sum_k CSF[k, j] x_iso[i, k])                     models.pyx:1264-1274
//     RESULTS['DWI_corrected'][mask == 1, :] = y_corrected * mean_b0 (b0 volumes kept)      core.py:488-498
// ONE streaming kernel in two output forms: rows f64[n][nS] (what AMX_F_CORRECTED writes) and the float32 volume [X][Y][Z][nS].
// It is a bandwidth row -- 4 bytes in, 4 (volume) or 8 (rows) bytes out per sample, ~24 bytes per voxel beside them --, so the lanes run
// along the FLATTENED (voxel, volume) index of a block of kCorrVox voxels that are consecutive in the C order of the volume: ranks follow
// that order, so the block's masked voxels have consecutive rows of y, and consecutive lanes read consecutive samples of y and write
// consecutive elements of the result, whatever nS is; voxels of few volumes share a wavefront.  (The 64 rank lookups of a block are
// strided when the image is Fortran-ordered -- the table is kept in the image's memory order --: 64 loads beside 4 160 samples.)  The
// isotropic columns of the dictionary (identical in every orientation's tile: taken from orientation 0) and the block's per-voxel
// values are staged in LDS once per workgroup; a sample costs one 32-bit division and n_iso fp64 LDS reads.  Measured, 300 000 masked of
// 360 000 voxels x 65 volumes, rescale + kept b0 columns: 0.058 ms, 3.0 TB/s of y + volume traffic (profiles/fw_corrected_rate.txt).
#include "amx_host.hpp"

namespace amx {

constexpr int kCorrVox = 64;       // voxels per workgroup (x nS samples: 16 per thread at 65 volumes)
constexpr int kCorrMaxIso = 8;     // isotropic atoms (the reference has one, Human, or two, Mouse)
constexpr int kCorrMaxB0 = 128;    // b0 columns that can be kept, like MAX_DEBIAS_B0

struct CorrArgs {
    const void *y;                 // T [n_vox][nS]
    const double *xiso;            // [n_vox][n_iso]
    const float *tile;             // orientation 0 of the dictionary: [nS][ldA], isotropic atoms in columns n_perp ..
    int nS, ldA, n_perp, n_iso;
    long long n_items;             // rows form: voxels; volume form: voxels of the whole volume
    // volume form
    const int *rank;               // [d2][d1][d0] in the image's memory-axis order: row of the voxel in y / xiso, or -1
    long long d[3], c[3];          // extents of the memory axes and their strides in the C-ordered volume
    const float *mean_b0;          // [n_vox] or null (no rescaling)
    unsigned keep[16];             // bit j: column j is a b0 volume that stays as it was (doKeepb0Intact)
    void *out;                     // rows: double [n_vox][nS]; volume: float [n_items][nS]
};

// fw, yc, the clip: fp64, products and sums rounded one by one in the reference's order.  hipcc contracts a * b + c into a fused
// multiply-add by default and its __dmul_rn / __dadd_rn are the plain operators, so contraction is switched off for these two functions.
__device__ __forceinline__ double corrected_sample(double y, const double *__restrict__ csf, const double *__restrict__ x, int n_iso)
{
#pragma clang fp contract(off)
    double fw = 0.0;
    for (int k = 0; k < n_iso; k++) { const double t = csf[k] * x[k]; fw = fw + t; }
    const double yc = y - fw;
    return yc < 0.0 ? 0.0 : yc;                                        // (NaN stays NaN)
}
__device__ __forceinline__ float scaled_sample(double v, double m)
{
#pragma clang fp contract(off)
    const double t = m * v;
    return (float)t;
}

template <typename T, bool VOLUME>
__global__ __launch_bounds__(256) void k_fw_corrected(const CorrArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_c[];
    const int nS = a.nS, n_iso = a.n_iso;
    double *csf = reinterpret_cast<double *>(smem_c);                   // [nS][n_iso]
    double *xs = csf + (size_t)nS * n_iso;                              // [kCorrVox][n_iso]
    double *ms = xs + kCorrVox * n_iso;                                 // [kCorrVox]
    int *rs = reinterpret_cast<int *>(ms + kCorrVox);                   // [kCorrVox]
    const long long v0 = (long long)blockIdx.x * kCorrVox;
    const int nv = (int)(a.n_items - v0 < kCorrVox ? a.n_items - v0 : kCorrVox);
    for (int e = threadIdx.x; e < nS * n_iso; e += blockDim.x) {
        const int j = e / n_iso, k = e - j * n_iso;
        csf[e] = (double)a.tile[(size_t)j * a.ldA + a.n_perp + k];
    }
    if ((int)threadIdx.x < nv) {
        const int t = threadIdx.x;
        long long r = v0 + t;
        if (VOLUME) {
            // C-order position -> coordinates along the image's memory axes -> the plan's rank table
            const long long cpos = v0 + t;
            const long long i0 = (cpos / a.c[0]) % a.d[0], i1 = (cpos / a.c[1]) % a.d[1], i2 = (cpos / a.c[2]) % a.d[2];
            r = a.rank[(i2 * a.d[1] + i1) * a.d[0] + i0];
            ms[t] = (r >= 0 && a.mean_b0) ? (double)a.mean_b0[r] : 1.0;
        }
        rs[t] = (int)r;
        for (int k = 0; k < n_iso; k++) xs[t * n_iso + k] = r >= 0 ? a.xiso[(size_t)r * n_iso + k] : 0.0;
    }
    __syncthreads();
    const unsigned total = (unsigned)nv * (unsigned)nS;
    const T *__restrict__ y = reinterpret_cast<const T *>(a.y);
    for (unsigned e = threadIdx.x; e < total; e += blockDim.x) {
        const unsigned t = e / (unsigned)nS;
        const int j = (int)(e - t * (unsigned)nS);
        const int r = rs[t];
        const size_t o = (size_t)v0 * nS + e;
        if (VOLUME) {
            float *out = reinterpret_cast<float *>(a.out);
            if (r < 0) { out[o] = 0.0f; continue; }
            const double yv = (double)y[(size_t)r * nS + j], m = ms[t];
            if ((a.keep[j >> 5] >> (j & 31)) & 1u) out[o] = scaled_sample(yv, m);                        // core.py:495-496
            else out[o] = scaled_sample(corrected_sample(yv, csf + j * n_iso, xs + t * n_iso, n_iso), m);  // core.py:493-494
        } else {
            reinterpret_cast<double *>(a.out)[o] = corrected_sample((double)y[o], csf + j * n_iso, xs + t * n_iso, n_iso);
        }
    }
}

}  // namespace amx

using namespace amx;

namespace {

int corr_common(amx_ctx *ctx, const amx_lut *lut, const char *who, CorrArgs &a)
{
    if (!lut || lut->model != 2 || lut->ctx != ctx) return amx_bad(ctx, (std::string(who) + ": not a FreeWater dictionary of this ctx").c_str());
    if (lut->n_iso > kCorrMaxIso) return amx_bad(ctx, (std::string(who) + ": more than 8 isotropic atoms").c_str());
    a.tile = reinterpret_cast<const float *>(lut->tiles);
    a.nS = lut->nS; a.ldA = lut->ldA; a.n_perp = lut->n_perp; a.n_iso = lut->n_iso;
    return AMX_OK;
}

size_t corr_lds(const CorrArgs &a) { return ((size_t)a.nS * a.n_iso + (size_t)kCorrVox * a.n_iso + kCorrVox) * sizeof(double) + kCorrVox * sizeof(int); }

template <typename K>
int corr_launch(amx_ctx *ctx, K kern, const CorrArgs &a, hipStream_t s)
{
    const long long blocks = (a.n_items + kCorrVox - 1) / kCorrVox;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), corr_lds(a), s, a);       // (at most 512 * 8 + 64 * 10 doubles: 38 KB)
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

}  // namespace

extern "C" {

int amx_freewater_corrected_device(amx_ctx *ctx, const amx_lut *lut, const float *d_y32, const double *d_y64, const double *d_xiso,
                                   int64_t n_vox, double *d_ycorr, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    CorrArgs a{};
    int rc;
    if ((rc = corr_common(ctx, lut, "amx_freewater_corrected", a))) return rc;
    if (n_vox < 0 || n_vox > INT_MAX / 4) return amx_bad(ctx, "amx_freewater_corrected: bad n_vox");
    if (n_vox == 0) return AMX_OK;
    if ((d_y32 == nullptr) == (d_y64 == nullptr) || !d_xiso || !d_ycorr) return amx_bad(ctx, "amx_freewater_corrected: need one of d_y32 / d_y64, d_xiso and d_ycorr");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    a.y = d_y32 ? (const void *)d_y32 : (const void *)d_y64; a.xiso = d_xiso; a.n_items = n_vox; a.out = d_ycorr;
    return d_y32 ? corr_launch(ctx, k_fw_corrected<float, false>, a, (hipStream_t)hip_stream)
                 : corr_launch(ctx, k_fw_corrected<double, false>, a, (hipStream_t)hip_stream);
}

int amx_prep_corrected_device(amx_ctx *ctx, const amx_prep *p, const amx_lut *lut, const float *d_y32, const double *d_xiso,
                              const float *d_mean_b0, const int32_t *b0_cols, int n_b0_cols, float *d_volume, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_corrected: not a plan of this ctx");
    CorrArgs a{};
    int rc;
    if ((rc = corr_common(ctx, lut, "amx_prep_corrected", a))) return rc;
    if (p->n_out != lut->nS) return amx_bad(ctx, "amx_prep_corrected: the plan prepares another number of volumes than the dictionary holds");
    if (!d_volume || (p->n_vox > 0 && (!d_y32 || !d_xiso))) return amx_bad(ctx, "amx_prep_corrected: null buffer");
    if (n_b0_cols < 0 || n_b0_cols > kCorrMaxB0 || (n_b0_cols > 0 && !b0_cols)) return amx_bad(ctx, "amx_prep_corrected: at most 128 b0 columns");
    for (int i = 0; i < n_b0_cols; i++) {
        if (b0_cols[i] < 0 || b0_cols[i] >= lut->nS) return amx_bad(ctx, "amx_prep_corrected: b0 column out of range");
        a.keep[b0_cols[i] >> 5] |= 1u << (b0_cols[i] & 31);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    a.y = d_y32; a.xiso = d_xiso; a.n_items = p->n_total; a.rank = p->rank; a.mean_b0 = d_mean_b0; a.out = d_volume;
    for (int k = 0; k < 3; k++) { a.d[k] = p->d[k]; a.c[k] = p->c[k]; }
    return corr_launch(ctx, k_fw_corrected<float, true>, a, (hipStream_t)hip_stream);
}

}  // extern "C"
