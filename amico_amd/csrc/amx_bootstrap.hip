// amx_bootstrap.hip -- the wild (residual) bootstrap of a fit's maps: what a replicate needs beside the fit itself.
//   k_boot_resample    y_b[i, j] = max(0, y_est[i, j] + s * (y[i, j] - y_est[i, j])), s = +-1 from a counter-based generator
//   k_boot_accumulate  Welford's running mean / M2 of the maps of the t-th replicate
//   k_boot_std         std = sqrt(M2 / (B - 1))
// All three are elementwise streams over a flat 64-bit index: no division, no LDS.  A lane takes kBootVec consecutive elements per trip
// (y: one 16-byte load as float, y_est: 32 bytes), the grid strides over the vectors, and the elements behind the last whole vector
// (or all of them, when a pointer is not 16-byte aligned) are walked one by one.  Arithmetic: fp64, every operation rounded on its
// own (no fused multiply-add), so the results equal the numpy restatement (tests/bootstrap_np.py) bit for bit.
// The sign of sample (voxel i, volume j) of replicate b is bit 63 of splitmix64's finaliser on
//     seed + (b + 1) * 0x9E3779B97F4A7C15 + ((first_voxel + i) * nS + j) * 0xD1B54A32D192ED03        (uint64, wraps)
// -- a function of (seed, b, first_voxel + i, j, nS) alone: not of n_vox, the launch shape or how a call is split.
#include "amx_host.hpp"

namespace amx {

constexpr int kBootVec = 4;          // consecutive elements per lane and trip
constexpr int kBootWaves = 8;        // workgroups per compute unit the grid is capped at (256 lanes each)

__device__ __forceinline__ bool boot_negative(unsigned long long key, unsigned long long ctr)
{
    unsigned long long z = key + ctr * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (z >> 63) != 0;
}

// v = y_est + s * r, r = y - y_est: s * r is exact, the two remaining operations are rounded one by one; the gather's clip (a NaN stays)
__device__ __forceinline__ double boot_sample(double y, double ye, bool neg)
{
#pragma clang fp contract(off)
    const double r = y - ye;
    const double sr = neg ? -r : r;
    const double v = ye + sr;
    return v < 0.0 ? 0.0 : v;
}

// kBootVec elements of y / y_b as 16-byte accesses (the host has checked that the pointers are 16-byte aligned)
struct BootQuad { double x, y, z, w; };
__device__ __forceinline__ BootQuad boot_load(const float *p, unsigned long long q)
{
    const float4 a = reinterpret_cast<const float4 *>(p)[q];
    return {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
}
__device__ __forceinline__ BootQuad boot_load(const double *p, unsigned long long q)
{
    const double2 a = reinterpret_cast<const double2 *>(p)[2 * q], b = reinterpret_cast<const double2 *>(p)[2 * q + 1];
    return {a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ void boot_store(float *p, unsigned long long q, const BootQuad &o)
{
    reinterpret_cast<float4 *>(p)[q] = make_float4((float)o.x, (float)o.y, (float)o.z, (float)o.w);
}
__device__ __forceinline__ void boot_store(double *p, unsigned long long q, const BootQuad &o)
{
    reinterpret_cast<double2 *>(p)[2 * q] = make_double2(o.x, o.y);
    reinterpret_cast<double2 *>(p)[2 * q + 1] = make_double2(o.z, o.w);
}

// n_vec whole vectors, then the elements [n_vec * kBootVec, total) one by one; ctr0 = first_voxel * nS
template <typename T>
__global__ __launch_bounds__(256) void k_boot_resample(const T *__restrict__ y, const double *__restrict__ ye, T *__restrict__ yb,
                                                       unsigned long long total, unsigned long long n_vec, unsigned long long key,
                                                       unsigned long long ctr0)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned long long q = tid; q < n_vec; q += stride) {
        const unsigned long long e = q * kBootVec;
        const BootQuad a = boot_load(y, q), p = boot_load(ye, q);
        BootQuad o;
        o.x = boot_sample(a.x, p.x, boot_negative(key, ctr0 + e));
        o.y = boot_sample(a.y, p.y, boot_negative(key, ctr0 + e + 1));
        o.z = boot_sample(a.z, p.z, boot_negative(key, ctr0 + e + 2));
        o.w = boot_sample(a.w, p.w, boot_negative(key, ctr0 + e + 3));
        boot_store(yb, q, o);
    }
    for (unsigned long long e = n_vec * kBootVec + tid; e < total; e += stride)
        yb[e] = (T)boot_sample((double)y[e], ye[e], boot_negative(key, ctr0 + e));
}

// Welford, the t-th value (t = 1 writes mean and M2 without reading them)
__device__ __forceinline__ void boot_welford(double m, double t, bool first, double &mean, double &m2)
{
#pragma clang fp contract(off)
    if (first) { mean = 0.0; m2 = 0.0; }
    const double d = m - mean;
    const double q = d / t;
    mean = mean + q;
    const double w = m - mean;
    const double p = d * w;
    m2 = m2 + p;
}

__global__ __launch_bounds__(256) void k_boot_accumulate(const double *__restrict__ maps, double *__restrict__ mean, double *__restrict__ m2,
                                                         unsigned long long total, unsigned long long n_vec, double t, int first)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned long long q = tid; q < n_vec; q += stride) {
        const double2 m = reinterpret_cast<const double2 *>(maps)[q];
        double2 a = make_double2(0.0, 0.0), s = make_double2(0.0, 0.0);
        if (!first) { a = reinterpret_cast<const double2 *>(mean)[q]; s = reinterpret_cast<const double2 *>(m2)[q]; }
        boot_welford(m.x, t, first, a.x, s.x);
        boot_welford(m.y, t, first, a.y, s.y);
        reinterpret_cast<double2 *>(mean)[q] = a;
        reinterpret_cast<double2 *>(m2)[q] = s;
    }
    for (unsigned long long e = n_vec * 2 + tid; e < total; e += stride) {
        double a = 0.0, s = 0.0;
        if (!first) { a = mean[e]; s = m2[e]; }
        boot_welford(maps[e], t, first, a, s);
        mean[e] = a; m2[e] = s;
    }
}

__global__ __launch_bounds__(256) void k_boot_std(const double *m2, double *sd, unsigned long long total, double denom)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const double v = m2[e] / denom;
        sd[e] = __dsqrt_rn(v);
    }
}

}  // namespace amx

using namespace amx;

namespace {

constexpr int64_t kBootMaxElems = (int64_t)1 << 46;      // elements of one call (far beyond any HBM; keeps every byte count in 63 bits)

unsigned boot_grid(const amx_ctx *ctx, unsigned long long work)
{
    const unsigned long long blocks = (work + 255) / 256, cap = (unsigned long long)(ctx->n_cu > 0 ? ctx->n_cu : 256) * kBootWaves;
    return (unsigned)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

bool boot_aligned(const void *p) { return ((uintptr_t)p & 15u) == 0; }

bool boot_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

template <typename T>
int boot_resample(amx_ctx *ctx, const T *d_y, const double *d_yest, int64_t n_vox, int nS, int64_t first_voxel, uint64_t seed,
                  int64_t replicate, T *d_yb, hipStream_t s)
{
    if (!ctx) return AMX_E_BADARG;
    if (nS < 1) return amx_bad(ctx, "amx_bootstrap_resample: bad nS");
    if (n_vox < 0 || n_vox > kBootMaxElems / nS) return amx_bad(ctx, "amx_bootstrap_resample: bad n_vox");
    if (first_voxel < 0 || replicate < 0) return amx_bad(ctx, "amx_bootstrap_resample: first_voxel and replicate must not be negative");
    if (n_vox == 0) return AMX_OK;
    if (!d_y || !d_yest || !d_yb) return amx_bad(ctx, "amx_bootstrap_resample: null buffer");
    const unsigned long long total = (unsigned long long)n_vox * (unsigned long long)nS;
    if (boot_overlap(d_yb, total * sizeof(T), d_y, total * sizeof(T)) || boot_overlap(d_yb, total * sizeof(T), d_yest, total * sizeof(double)))
        return amx_bad(ctx, "amx_bootstrap_resample: d_yb must not overlap d_y or d_yest");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const unsigned long long n_vec = (boot_aligned(d_y) && boot_aligned(d_yest) && boot_aligned(d_yb)) ? total / kBootVec : 0;
    const unsigned long long key = seed + ((unsigned long long)replicate + 1ull) * 0x9E3779B97F4A7C15ull;
    const unsigned long long ctr0 = (unsigned long long)first_voxel * (unsigned long long)nS;
    hipLaunchKernelGGL(k_boot_resample<T>, dim3(boot_grid(ctx, n_vec ? n_vec : total)), dim3(256), 0, s, d_y, d_yest, d_yb, total, n_vec, key, ctr0);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

}  // namespace

extern "C" {

int amx_bootstrap_resample_device(amx_ctx *ctx, const double *d_y, const double *d_yest, int64_t n_vox, int nS, int64_t first_voxel,
                                  uint64_t seed, int64_t replicate, double *d_yb, void *hip_stream)
{
    return boot_resample<double>(ctx, d_y, d_yest, n_vox, nS, first_voxel, seed, replicate, d_yb, (hipStream_t)hip_stream);
}

int amx_bootstrap_resample_device_f32(amx_ctx *ctx, const float *d_y, const double *d_yest, int64_t n_vox, int nS, int64_t first_voxel,
                                      uint64_t seed, int64_t replicate, float *d_yb, void *hip_stream)
{
    return boot_resample<float>(ctx, d_y, d_yest, n_vox, nS, first_voxel, seed, replicate, d_yb, (hipStream_t)hip_stream);
}

int amx_bootstrap_accumulate_device(amx_ctx *ctx, const double *d_maps, int64_t n_elems, int64_t t, double *d_mean, double *d_m2,
                                    void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (n_elems < 0 || n_elems > kBootMaxElems) return amx_bad(ctx, "amx_bootstrap_accumulate: bad n_elems");
    if (t < 1) return amx_bad(ctx, "amx_bootstrap_accumulate: t counts the replicates from 1");
    if (n_elems == 0) return AMX_OK;
    if (!d_maps || !d_mean || !d_m2) return amx_bad(ctx, "amx_bootstrap_accumulate: null buffer");
    const size_t bytes = (size_t)n_elems * sizeof(double);
    if (boot_overlap(d_mean, bytes, d_m2, bytes) || boot_overlap(d_mean, bytes, d_maps, bytes) || boot_overlap(d_m2, bytes, d_maps, bytes))
        return amx_bad(ctx, "amx_bootstrap_accumulate: d_maps, d_mean and d_m2 must not overlap");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const unsigned long long total = (unsigned long long)n_elems;
    const unsigned long long n_vec = (boot_aligned(d_maps) && boot_aligned(d_mean) && boot_aligned(d_m2)) ? total / 2 : 0;
    hipLaunchKernelGGL(k_boot_accumulate, dim3(boot_grid(ctx, n_vec ? n_vec : total)), dim3(256), 0, (hipStream_t)hip_stream, d_maps, d_mean,
                       d_m2, total, n_vec, (double)t, t == 1 ? 1 : 0);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

int amx_bootstrap_std_device(amx_ctx *ctx, const double *d_m2, int64_t n_elems, int64_t B, double *d_std, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (n_elems < 0 || n_elems > kBootMaxElems) return amx_bad(ctx, "amx_bootstrap_std: bad n_elems");
    if (B < 2) return amx_bad(ctx, "amx_bootstrap_std: the standard deviation needs at least 2 replicates");
    if (n_elems == 0) return AMX_OK;
    if (!d_m2 || !d_std) return amx_bad(ctx, "amx_bootstrap_std: null buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_boot_std, dim3(boot_grid(ctx, (unsigned long long)n_elems)), dim3(256), 0, (hipStream_t)hip_stream, d_m2, d_std,
                       (unsigned long long)n_elems, (double)(B - 1));
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

}  // extern "C"
