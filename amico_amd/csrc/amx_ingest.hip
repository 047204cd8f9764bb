// amx_ingest.hip -- the image in its STORED dtype -> the float32 image of core.py:136 (`niiDWI_img = img.astype(np.float32)`, with the
// NIfTI header's scl_slope / scl_inter applied the way nibabel applies them), fused with the NaN / Inf scan of core.py:152-158 that
// is the first kernel of the chain otherwise: the raw bytes are read once, every float32 element is written once.
//
// Value rule (the reference is numpy):
//   no scaling   out = np.float32(raw)                               int32 and float64 round to nearest even, float64 beyond float32's
//                                                                    range -> +-Inf, denormals and -0.0 stay, float32 keeps its bits
//   scaling      out = np.float32(np.float64(raw) * slope + inter)   product and sum each rounded in fp64: contraction is off
// The scan is amx_sanitize.hip's, on the integer pattern of the float32 RESULT: every exponent bit set -> counted, and with `replace`
// overwritten with `value` before it is stored.
//
//   k_ingest<T, SCALED>   `count` contiguous elements.  A lane's step is kStep elements: 16 bytes of uint8 / int16 / uint16 / int32 /
//                         float32, two 16-byte loads of float64 -> 4, 2, 1, 1 stores of 16 bytes.  `head` elements put the float32
//                         stores on a 16-byte boundary.  The raw loads are 16 bytes wide wherever the block starts: their type carries
//                         the element's alignment only, and global memory takes such an access at any address (both buffers at the
//                         start of an allocation: loads and stores are all on 16-byte boundaries).  Head and tail elements go one
//                         per lane to block 0.
#include "amx_sanitize.hpp"
#include <cmath>
#include <type_traits>

namespace amx {

struct alignas(16) IngestVec { unsigned int x, y, z, w; };          // one 16-byte store of four float32 patterns
// 16 bytes of raw elements, aligned like ONE of them: a block of 2-byte elements may start at any multiple of 2 bytes
template <int A> struct IngestRaw;
template <> struct IngestRaw<1> { typedef unsigned int type __attribute__((ext_vector_type(4), aligned(1))); };
template <> struct IngestRaw<2> { typedef unsigned int type __attribute__((ext_vector_type(4), aligned(2))); };
template <> struct IngestRaw<4> { typedef unsigned int type __attribute__((ext_vector_type(4), aligned(4))); };
template <> struct IngestRaw<8> { typedef unsigned int type __attribute__((ext_vector_type(4), aligned(8))); };

template <typename T> struct IngestStep { static constexpr int kStep = 16 / (int)sizeof(T); };
template <> struct IngestStep<double> { static constexpr int kStep = 4; };

// one element by the value rule, as the bits of its float32.  hipcc contracts a * b + c into a fused multiply-add by default
// (amx_fw_corrected.hip), which rounds once where numpy rounds twice.
template <typename T, bool SCALED>
__device__ __forceinline__ unsigned int ingest_bits(T x, double slope, double inter)
{
#pragma clang fp contract(off)
    if constexpr (SCALED) {
        const double r = (double)x;
        const double t = r * slope;
        const double u = t + inter;
        return __float_as_uint((float)u);
    } else if constexpr (sizeof(T) == 4 && !std::is_integral<T>::value) {
        return __float_as_uint(x);                        // float32 as it is, NaN payloads included
    } else {
        return __float_as_uint((float)x);
    }
}

// scan of core.py:152-158 on the result: -> 1 when it was non-finite (and `b` holds the replacement when asked to)
__device__ __forceinline__ unsigned int ingest_scan(unsigned int &b, int replace, unsigned int value_bits)
{
    if ((b & 0x7f800000u) != 0x7f800000u) return 0u;
    if (replace) b = value_bits;
    return 1u;
}

template <typename T, bool SCALED>
__global__ __launch_bounds__(256) void k_ingest(const T *__restrict__ raw, float *__restrict__ out, long long head, long long nstep,
                                                long long tail, double slope, double inter, int replace, unsigned int value_bits,
                                                unsigned long long *counter)
{
    constexpr int E = IngestStep<T>::kStep, NL = E * (int)sizeof(T) / 16, NS = E / 4;
    typedef typename IngestRaw<(int)sizeof(T)>::type RawVec;
    union Step { RawVec w[NL]; T v[E]; };
    const T *rp = raw + head;
    IngestVec *op = reinterpret_cast<IngestVec *>(out + head);             // 16-byte aligned by the choice of `head`
    unsigned int mine = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nstep; i += 2 * stride) {
        Step in[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const long long j = i + k * stride;
            if (j < nstep) {
                const RawVec *q = reinterpret_cast<const RawVec *>(rp + j * E);
#pragma unroll
                for (int l = 0; l < NL; l++) in[k].w[l] = q[l];
            }
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const long long j = i + k * stride;
            if (j < nstep) {
#pragma unroll
                for (int q = 0; q < NS; q++) {
                    unsigned int b[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        b[e] = ingest_bits<T, SCALED>(in[k].v[4 * q + e], slope, inter);
                        mine += ingest_scan(b[e], replace, value_bits);
                    }
                    op[j * NS + q] = IngestVec{b[0], b[1], b[2], b[3]};
                }
            }
        }
    }
    if (blockIdx.x == 0) {
        const long long t = threadIdx.x;                           // head < 4 and tail < kStep <= 16: one lane each
        unsigned int *o = reinterpret_cast<unsigned int *>(out);
        if (t < head) {
            unsigned int b = ingest_bits<T, SCALED>(raw[t], slope, inter);
            mine += ingest_scan(b, replace, value_bits);
            o[t] = b;
        }
        if (t < tail) {
            const long long at = head + nstep * E + t;
            unsigned int b = ingest_bits<T, SCALED>(raw[at], slope, inter);
            mine += ingest_scan(b, replace, value_bits);
            o[at] = b;
        }
    }
    san_block_add(mine, counter);
}

}  // namespace amx

using namespace amx;

namespace {

template <typename T> const char *ingest_name(bool scaled);
#define AMX_INGEST_NAME(T, tag)                                                                                     \
    template <> const char *ingest_name<T>(bool scaled) { return scaled ? "k_ingest<" tag ",scaled>" : "k_ingest<" tag ">"; }
AMX_INGEST_NAME(unsigned char, "u8")
AMX_INGEST_NAME(short, "i16")
AMX_INGEST_NAME(unsigned short, "u16")
AMX_INGEST_NAME(int, "i32")
AMX_INGEST_NAME(float, "f32")
AMX_INGEST_NAME(double, "f64")
#undef AMX_INGEST_NAME

template <typename T>
int ingest_flat(amx_ctx *ctx, const void *d_raw, long long count, bool scaled, double slope, double inter, int replace, float value,
                float *d_img, hipStream_t s)
{
    constexpr int E = IngestStep<T>::kStep;
    if ((uintptr_t)d_raw % sizeof(T)) return amx_bad(ctx, "amx_prep_ingest: the raw buffer is not aligned to its element size");
    if ((uintptr_t)d_img % 4) return amx_bad(ctx, "amx_prep_ingest: the image buffer is not aligned to 4 bytes");
    const uintptr_t r0 = (uintptr_t)d_raw, r1 = r0 + (uintptr_t)count * sizeof(T), o0 = (uintptr_t)d_img, o1 = o0 + (uintptr_t)count * 4;
    if (r0 < o1 && o0 < r1) return amx_bad(ctx, "amx_prep_ingest: the raw buffer and the image overlap");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long *counter;
    int rc;
    if ((rc = san_begin(ctx, s, &counter))) return rc;
    const T *raw = static_cast<const T *>(d_raw);
    long long head = (long long)(((16 - ((uintptr_t)d_img & 15)) & 15) / 4);
    if (head > count) head = count;
    const long long nstep = (count - head) / E, tail = count - head - nstep * E;
    unsigned int vb;
    memcpy(&vb, &value, sizeof vb);
    const dim3 grid(san_grid(ctx, (nstep + 1) / 2)), block(256);
    const int rep = replace ? 1 : 0;
    if (scaled) hipLaunchKernelGGL((k_ingest<T, true>), grid, block, 0, s, raw, d_img, head, nstep, tail, slope, inter, rep, vb, counter);
    else        hipLaunchKernelGGL((k_ingest<T, false>), grid, block, 0, s, raw, d_img, head, nstep, tail, slope, inter, rep, vb, counter);
    return san_end(ctx, s, ingest_name<T>(scaled));
}

size_t ingest_elem(int raw_dtype)
{
    switch (raw_dtype) {
    case AMX_T_U8: return 1;
    case AMX_T_I16: case AMX_T_U16: return 2;
    case AMX_T_I32: case AMX_T_F32: return 4;
    case AMX_T_F64: return 8;
    }
    return 0;
}

}  // namespace

extern "C" {

int amx_prep_ingest_device(amx_ctx *ctx, const amx_prep *p, const void *d_raw, int raw_dtype, double slope, double inter, int replace,
                           float value, float *d_img, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_ingest: not a plan of this ctx");
    if (!d_raw || !d_img) return amx_bad(ctx, "amx_prep_ingest: null buffer");
    if (!ingest_elem(raw_dtype)) return amx_bad(ctx, "amx_prep_ingest: raw_dtype must be one of AMX_T_U8 / I16 / U16 / I32 / F32 / F64");
    if (!std::isfinite(slope) || !std::isfinite(inter)) return amx_bad(ctx, "amx_prep_ingest: slope and inter must be finite");
    if (replace && !std::isfinite(value)) return amx_bad(ctx, "amx_prep_ingest: the replacement value must be finite");
    long long d[4], st[4];
    if (!san_axes(p, d, st))
        return amx_bad(ctx, "amx_prep_ingest: the plan's image is not a permutation of a contiguous block (a view with gaps); convert it on the host");
    const bool scaled = !(slope == 1.0 && inter == 0.0);
    hipStream_t s = (hipStream_t)hip_stream;
    switch (raw_dtype) {
    case AMX_T_U8:  return ingest_flat<unsigned char>(ctx, d_raw, p->extent, scaled, slope, inter, replace, value, d_img, s);
    case AMX_T_I16: return ingest_flat<short>(ctx, d_raw, p->extent, scaled, slope, inter, replace, value, d_img, s);
    case AMX_T_U16: return ingest_flat<unsigned short>(ctx, d_raw, p->extent, scaled, slope, inter, replace, value, d_img, s);
    case AMX_T_I32: return ingest_flat<int>(ctx, d_raw, p->extent, scaled, slope, inter, replace, value, d_img, s);
    case AMX_T_F32: return ingest_flat<float>(ctx, d_raw, p->extent, scaled, slope, inter, replace, value, d_img, s);
    default:        return ingest_flat<double>(ctx, d_raw, p->extent, scaled, slope, inter, replace, value, d_img, s);
    }
}

int amx_prep_ingest(amx_ctx *ctx, const amx_prep *p, const void *raw, int raw_dtype, double slope, double inter, int replace, float value,
                    float *img, int64_t *out_count)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_ingest: not a plan of this ctx");
    if (!raw || !img || !out_count) return amx_bad(ctx, "amx_prep_ingest: null argument");
    const size_t eb = ingest_elem(raw_dtype);
    if (!eb) return amx_bad(ctx, "amx_prep_ingest: raw_dtype must be one of AMX_T_U8 / I16 / U16 / I32 / F32 / F64");
    *out_count = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t rb = (size_t)p->extent * eb, ib = (size_t)p->extent * sizeof(float);
    if ((rc = amx_ensure(ctx, ctx->hy, rb))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hextra, ib))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->hy.p, raw, rb, hipMemcpyHostToDevice, nullptr));
    if ((rc = amx_prep_ingest_device(ctx, p, ctx->hy.p, raw_dtype, slope, inter, replace, value, (float *)ctx->hextra.p, nullptr))) return rc;
    if ((rc = amx_sanitize_last(ctx, out_count))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(img, ctx->hextra.p, ib, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}

}  // extern "C"
