// amx_sanitize.hip -- find (and replace) the NaN / Inf samples of a signal buffer: core.py:152-158 (raw image) and core.py:270-276
// (pre-processed image) of load_data(..., replace_bad_voxels).  The reference tests `np.isnan(img).any() or np.isinf(img).any()` and
// either refuses or calls np.nan_to_num(img, copy=False, nan=r, posinf=r, neginf=r): NaN, +Inf and -Inf all become float32(r) and
// every finite element keeps its bits.
//
//   k_sanitize_flat     `count` contiguous elements (float | double): grid-stride loop of 16-byte loads, four in flight per lane; the
//                       elements ahead of the first 16-byte boundary and behind the last whole vector go one per lane to block 0
//   k_sanitize_strided  the float32 image of a plan that is NOT a permutation of a contiguous block (a view with gaps): one lane per
//                       element of the image, walked with its fastest axis innermost; memory between the elements is never touched
//
// Non-finite = all exponent bits set, tested on the integer pattern (no floating-point compare a fast-math build could fold away).
// A vector is stored back only when it held a bad element: on clean data the kernels read and never write.  Counting: per lane ->
// wavefront (shuffle sum) -> block (LDS) -> ONE 64-bit atomicAdd per block that found something, into a device counter that the
// launch function zeroes on the same stream and copies to pinned host memory behind the kernel.  The ctx keeps two counters with an event each and alternates between them, so the counts
// of the last TWO calls can be read (amx_sanitize_last / amx_sanitize_previous): a chain enqueues the image scan and the scan of y on
// one stream and reads both after its only wait.
#include "amx_sanitize.hpp"
#include <cmath>

namespace amx {

template <typename T> struct SanBits;
template <> struct SanBits<float> {
    typedef unsigned int U;
    static constexpr U kExp = 0x7f800000u;
    static constexpr int kPerVec = 4;
};
template <> struct SanBits<double> {
    typedef unsigned long long U;
    static constexpr U kExp = 0x7ff0000000000000ull;
    static constexpr int kPerVec = 2;
};

// one element through its integer pattern; returns 1 when it was bad (and has been replaced when asked to)
template <typename U>
__device__ __forceinline__ unsigned int san_scalar(U *p, U exp_mask, int replace, U value_bits)
{
    const U b = *p;
    if ((b & exp_mask) != exp_mask) return 0u;
    if (replace) *p = value_bits;
    return 1u;
}

template <typename T>
__global__ __launch_bounds__(256) void k_sanitize_flat(T *buf, long long head, long long nvec, long long tail, int replace,
                                                       typename SanBits<T>::U value_bits, unsigned long long *counter)
{
    typedef typename SanBits<T>::U U;
    constexpr U kExp = SanBits<T>::kExp;
    constexpr int V = SanBits<T>::kPerVec;
    U *w = reinterpret_cast<U *>(buf);
    // 16-byte aligned by the choice of `head` (float64 elements that sit on odd multiples of 4 bytes never reach such a boundary: their
    // vectors are dword-aligned multi-dword accesses, which the memory pipeline takes at a lower rate)
    uint4 *vec = reinterpret_cast<uint4 *>(w + head);
    unsigned int mine = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += 4 * stride) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const long long j = i + k * stride;
            v[k] = j < nvec ? vec[j] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            unsigned int bad = 0;
            if constexpr (V == 4) {
                unsigned int *e = reinterpret_cast<unsigned int *>(&v[k]);
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if ((e[q] & (unsigned int)kExp) == (unsigned int)kExp) { bad++; e[q] = (unsigned int)value_bits; }
            } else {
                // little endian: the high word of each double holds its exponent
                unsigned int *e = reinterpret_cast<unsigned int *>(&v[k]);
                const unsigned int hi = (unsigned int)((unsigned long long)kExp >> 32);
#pragma unroll
                for (int q = 0; q < 2; q++)
                    if ((e[2 * q + 1] & hi) == hi) {
                        bad++;
                        e[2 * q] = (unsigned int)((unsigned long long)value_bits & 0xffffffffull);
                        e[2 * q + 1] = (unsigned int)((unsigned long long)value_bits >> 32);
                    }
            }
            if (bad) {
                mine += bad;
                if (replace) vec[i + k * stride] = v[k];       // (bad != 0 implies the vector was in range)
            }
        }
    }
    if (blockIdx.x == 0) {
        const long long t = threadIdx.x;
        if (t < head) mine += san_scalar<U>(w + t, kExp, replace, value_bits);
        if (t < tail) mine += san_scalar<U>(w + head + nvec * V + t, kExp, replace, value_bits);
    }
    san_block_add(mine, counter);
}

struct SanStrided {
    float *img;
    long long d[4], s[4];         // extents and element strides of the four axes, d[0] / s[0] the fastest in memory
    long long total;
};

__global__ __launch_bounds__(256) void k_sanitize_strided(SanStrided a, int replace, unsigned int value_bits, unsigned long long *counter)
{
    unsigned int mine = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += stride) {
        const long long i0 = i % a.d[0], r0 = i / a.d[0], i1 = r0 % a.d[1], r1 = r0 / a.d[1], i2 = r1 % a.d[2], i3 = r1 / a.d[2];
        unsigned int *p = reinterpret_cast<unsigned int *>(a.img + (i0 * a.s[0] + i1 * a.s[1] + i2 * a.s[2] + i3 * a.s[3]));
        mine += san_scalar<unsigned int>(p, 0x7f800000u, replace, value_bits);
    }
    san_block_add(mine, counter);
}

}  // namespace amx

using namespace amx;

namespace {

template <typename T>
int sanitize_flat(amx_ctx *ctx, T *d_buf, int64_t count, int replace, T value, hipStream_t s, const char *who)
{
    typedef typename SanBits<T>::U U;
    if (count < 0) return amx_bad(ctx, "amx_sanitize: negative count");
    if (replace && !std::isfinite(value)) return amx_bad(ctx, "amx_sanitize: the replacement value must be finite");
    if (count > 0 && !d_buf) return amx_bad(ctx, "amx_sanitize: null buffer");
    if ((uintptr_t)d_buf % 4) return amx_bad(ctx, "amx_sanitize: the buffer is not aligned to 4 bytes");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long *counter;
    int rc;
    if ((rc = san_begin(ctx, s, &counter))) return rc;
    if (count > 0) {
        constexpr int V = SanBits<T>::kPerVec;
        long long head = (long long)(((16 - ((uintptr_t)d_buf & 15)) & 15) / sizeof(T));
        if (head > count) head = count;
        const long long nvec = (count - head) / V, tail = count - head - nvec * V;
        U vb;
        memcpy(&vb, &value, sizeof vb);
        hipLaunchKernelGGL((k_sanitize_flat<T>), dim3(san_grid(ctx, (nvec + 3) / 4)), dim3(256), 0, s, d_buf, head, nvec, tail, replace ? 1 : 0, vb, counter);
    }
    return san_end(ctx, s, who);
}

}  // namespace

extern "C" {

int amx_sanitize_device_f32(amx_ctx *ctx, float *d_buf, int64_t count, int replace, float value, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    return sanitize_flat<float>(ctx, d_buf, count, replace, value, (hipStream_t)hip_stream, "k_sanitize_flat<f32>");
}

int amx_sanitize_device(amx_ctx *ctx, double *d_buf, int64_t count, int replace, double value, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    return sanitize_flat<double>(ctx, d_buf, count, replace, value, (hipStream_t)hip_stream, "k_sanitize_flat<f64>");
}

int amx_prep_sanitize_device(amx_ctx *ctx, const amx_prep *p, float *d_img, int replace, float value, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_sanitize: not a plan of this ctx");
    if (!d_img) return amx_bad(ctx, "amx_prep_sanitize: null buffer");
    SanStrided a;
    a.img = d_img;
    if (san_axes(p, a.d, a.s))       // a permutation of a contiguous block: every element of the extent is the image's
        return sanitize_flat<float>(ctx, d_img, p->extent, replace, value, (hipStream_t)hip_stream, "k_sanitize_flat<f32>");
    if (replace && !std::isfinite(value)) return amx_bad(ctx, "amx_sanitize: the replacement value must be finite");
    if ((uintptr_t)d_img % 4) return amx_bad(ctx, "amx_sanitize: the buffer is not aligned to 4 bytes");
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    a.total = p->n_total * p->nS;
    unsigned long long *counter;
    int rc;
    if ((rc = san_begin(ctx, s, &counter))) return rc;
    unsigned int vb;
    memcpy(&vb, &value, sizeof vb);
    hipLaunchKernelGGL(k_sanitize_strided, dim3(san_grid(ctx, a.total)), dim3(256), 0, s, a, replace ? 1 : 0, vb, counter);
    return san_end(ctx, s, "k_sanitize_strided");
}

static int san_read(amx_ctx *ctx, unsigned back, int64_t *out, const char *who)
{
    if (!ctx) return AMX_E_BADARG;
    if (!out) return amx_bad(ctx, who);
    *out = 0;
    if (!ctx->san_count || ctx->san_seq < back) return AMX_OK;
    const int slot = (int)((ctx->san_seq - back) & 1u);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize(ctx->san_ev[slot]));
    *out = (int64_t)ctx->san_host[slot];
    return AMX_OK;
}

int amx_sanitize_last(amx_ctx *ctx, int64_t *out_count) { return san_read(ctx, 1, out_count, "amx_sanitize_last: null output"); }

int amx_sanitize_previous(amx_ctx *ctx, int64_t *out_count) { return san_read(ctx, 2, out_count, "amx_sanitize_previous: null output"); }

int amx_sanitize(amx_ctx *ctx, double *buf, int64_t count, int replace, double value, int64_t *out_count)
{
    if (!ctx) return AMX_E_BADARG;
    if (count < 0 || !out_count || (count > 0 && !buf)) return amx_bad(ctx, "amx_sanitize: bad argument");
    *out_count = 0;
    if (replace && !std::isfinite(value)) return amx_bad(ctx, "amx_sanitize: the replacement value must be finite");
    if (count == 0) return AMX_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t nb = (size_t)count * sizeof(double);
    if ((rc = amx_ensure(ctx, ctx->hy, nb))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->hy.p, buf, nb, hipMemcpyHostToDevice, nullptr));
    if ((rc = amx_sanitize_device(ctx, (double *)ctx->hy.p, count, replace, value, nullptr))) return rc;
    if ((rc = amx_sanitize_last(ctx, out_count))) return rc;
    if (replace && *out_count > 0) {
        HIPCHK(ctx, hipMemcpyAsync(buf, ctx->hy.p, nb, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(ctx, hipStreamSynchronize(nullptr));
    }
    return AMX_OK;
}

int amx_prep_sanitize(amx_ctx *ctx, const amx_prep *p, float *img, int replace, float value, int64_t *out_count)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_sanitize: not a plan of this ctx");
    if (!img || !out_count) return amx_bad(ctx, "amx_prep_sanitize: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t ib = (size_t)p->extent * sizeof(float);
    if ((rc = amx_ensure(ctx, ctx->hextra, ib))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->hextra.p, img, ib, hipMemcpyHostToDevice, nullptr));
    if ((rc = amx_prep_sanitize_device(ctx, p, (float *)ctx->hextra.p, replace, value, nullptr))) return rc;
    if ((rc = amx_sanitize_last(ctx, out_count))) return rc;
    if (replace && *out_count > 0) {       // (elements of the extent that are not the image's come back as they went)
        HIPCHK(ctx, hipMemcpyAsync(img, ctx->hextra.p, ib, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(ctx, hipStreamSynchronize(nullptr));
    }
    return AMX_OK;
}

}  // extern "C"
