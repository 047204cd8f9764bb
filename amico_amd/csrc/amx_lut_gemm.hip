// amx_lut_gemm.hip -- LUT resampling (SURVEY section 8 f, row 4)
// lut.pyx:274-311 `resample_kernel`:  KR = ones(ndirs, nS);  KR[i, idx_out] = dot(Ylm_out, KRlm[i, :])  for every
// orientation i -- batched over all atoms as ONE float32 GEMM  C[M x N] = L[M x K] * Ylm^T[K x N]  (M = atoms * ndirs rows
// of rotated SH coefficients, K = nSH * shells, N = number of DWI volumes) on the matrix cores.
#include "amx_host.hpp"
#include "amx_lut_route.hpp"

using namespace amx;

namespace amx {

typedef float floatx16 __attribute__((ext_vector_type(16)));

__global__ void k_fill_ones(float *out, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = 1.0f;
}

// Shapes whose SH -> signal operator fits the LDS (K <= 256 reduction indices; NODDI / FreeWater: K = 182, N = 90).
// One wavefront = 32 rows of L against all N columns, 32 at a time, with v_mfma_f32_32x32x2_f32.  The reduction index is
// split in two halves, one per half-wavefront (lane l works on k = (l / 32) * 2 KH2 + j): every lane owns a contiguous
// half row of L, held in registers for all column tiles, and a half row of Ylm in LDS (N x K floats staged once per
// workgroup, read with ds_read_b64; the row stride has an odd number of 8-byte words: 32 rows hit all 64 banks).
// KH2 = pairs per half-wavefront, a compile-time bound: the loops carry no conditions (indices beyond K read zeros).
// The order of a sum does not matter to the GEMM.  Measured for 72 000 x 182 x 90 (profiles/): 0.093 ms = 25 TFLOP/s, 16 %
// of the f32 matrix peak (0.35 ms before); variants that did NOT help: the rows of L through a coalesced per-wavefront
// LDS tile (0.13 ms at one workgroup per CU), three independent accumulators (0.10 ms, one wavefront per SIMD).
// (kLutKhMax and the arithmetic that picks one of the three kernels: amx_lut_route.hpp)

// Fused mode (Z != nullptr, amx_lut_rotate_resample): row (atom, orientation) of L is never materialised --
// L[atom * ndirs + dir][k] = Z[atom][k] * R[dir][k mod n_sh]  (rotate_kernel, lut.pyx:262-264: const * Klm[idx_m0] * Ylm_rot).
template <int KH2>
__global__ __launch_bounds__(256) void k_lut_resample(const float *__restrict__ L, const float *__restrict__ Y,
                                                      const int *__restrict__ idx_out, long long M, int K, int N, int nS,
                                                      float *__restrict__ out, const float *__restrict__ Z = nullptr,
                                                      const float *__restrict__ R = nullptr, int ndirs = 1, int n_sh = 1)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_l[];
    constexpr int Kp = 4 * KH2;                                      // padded K
    constexpr int Ks = Kp + 2;                                       // Ylm row stride (floats): Ks / 2 odd
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int Npad = (N + 31) & ~31;
    float *Ys = reinterpret_cast<float *>(smem_l);                    // [Npad][Ks], zero padded
    // (rows by wavefront, columns by lane, eight rows of loads in flight)
    for (int nb = wave * 8; nb < Npad; nb += 32) {
        for (int k = lane; k < Ks; k += 64) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int n = nb + u;
                t[u] = (n < N && k < K) ? Y[(long long)n * K + k] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (nb + u < Npad) Ys[(size_t)(nb + u) * Ks + k] = t[u];
        }
    }
    __syncthreads();
    const bool even = (K & 1) == 0;                                  // rows of L start 8-byte aligned
    for (long long m0 = ((long long)blockIdx.x * 4 + wave) * 32; m0 < M; m0 += (long long)gridDim.x * 128) {
        // this lane's half row of L, loaded once with 8-byte loads (rows beyond M repeat the last one; masked at the store)
        const long long row = m0 + l32 < M ? m0 + l32 : M - 1;
        float2 a2[KH2];
        if (Z == nullptr) {
            const float *lrow = L + row * K;
#pragma unroll
            for (int j = 0; j < KH2; j++) {
                const int k = 2 * half * KH2 + 2 * j;
                if (even && 2 * KH2 + 2 * j + 1 < K) {               // (holds for both halves: no condition per lane)
                    a2[j] = *reinterpret_cast<const float2 *>(lrow + k);
                } else {
                    a2[j].x = (k < K) ? lrow[k] : 0.0f;
                    a2[j].y = (k + 1 < K) ? lrow[k + 1] : 0.0f;
                }
            }
        } else {
            // rotation by the addition theorem, formed in registers: per-(l, m) factor of the atom x basis value of the orientation
            const float *zrow = Z + (row / ndirs) * K, *rrow = R + (row % ndirs) * n_sh;
            int c = (2 * half * KH2) % n_sh;                          // position inside the shell's block of coefficients
#pragma unroll
            for (int j = 0; j < KH2; j++) {
                const int k = 2 * half * KH2 + 2 * j;
                const int c1 = (c + 1 == n_sh) ? 0 : c + 1;
                a2[j].x = (k < K) ? zrow[k] * rrow[c] : 0.0f;
                a2[j].y = (k + 1 < K) ? zrow[k + 1] * rrow[c1] : 0.0f;
                c = (c1 + 1 == n_sh) ? 0 : c1 + 1;
            }
        }
        for (int n0 = 0; n0 < N; n0 += 32) {
            const float2 *yrow = reinterpret_cast<const float2 *>(Ys + (size_t)(n0 + l32) * Ks + 2 * half * KH2);
            floatx16 acc;
#pragma unroll
            for (int i = 0; i < 16; i++) acc[i] = 0.0f;
#pragma unroll
            for (int j = 0; j < KH2; j++) {
                const float2 b2 = yrow[j];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[j].x, b2.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[j].y, b2.y, acc, 0, 0, 0);
            }
            const int n = n0 + l32;
            if (n < N) {
                const int col = idx_out[n];
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const long long r = m0 + 8 * (i / 4) + 4 * half + (i % 4);
                    if (r < M) out[r * nS + col] = acc[i];
                }
            }
        }
    }
}

// The same GEMM with BOTH operands in LDS (plain `lm` input, K even, operator + four row tiles <= 160 KB): what limited
// k_lut_resample was not the matrix pipe but its left operand -- every lane walking its own 728-byte row of L with 8-byte
// loads (64 cache lines per load instruction: 59 % of the wavefronts' time, matrix pipe 18 % busy).  32 consecutive rows of L
// are ONE contiguous 23 KB block, so a wavefront streams its tile global -> LDS with direct 16-byte loads (23 instructions,
// all in flight at once) and reads the MFMA operand from there; the row stride K = 182 floats puts 32 consecutive rows into
// 32 different even banks, for the tile and for the operator alike, so neither needs padding or a swizzle.  A row is read up
// to 4 KH2 - K floats beyond its end (the next row: finite values); the left operand is forced to zero there.
#ifdef AMX_LUT_PHASES
__device__ unsigned long long g_lut_ph[8];
#define LPH_T() __builtin_readcyclecounter()
#define LPH_ADD(k, t0) ph[k] += __builtin_readcyclecounter() - (t0)
#else
#define LPH_T() 0ull
#define LPH_ADD(k, t0) (void)(t0)
#endif
template <int KH2>
__global__ __launch_bounds__(256) void k_lut_resample_tile(const float *__restrict__ L, const float *__restrict__ Y,
                                                           const int *__restrict__ idx_out, long long M, int K, int N, int nS,
                                                           float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_t[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, l32 = lane & 31;
#ifdef AMX_LUT_PHASES
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long t_all = LPH_T();
#endif
    unsigned long long t0 = LPH_T();
    // LDS: Ys [N][K] (+ a zeroed tail of 1056 B) | per wavefront: Lt [32][K]
    float *Ys = reinterpret_cast<float *>(smem_t);
    const long long ybytes = (long long)N * K * 4;
    const long long yzone = ((ybytes + 1023) & ~1023LL) + 2048;      // the copy's last piece ends inside; rows N .. N + 31 start inside or behind
    const long long tile_bytes = 32LL * K * 4, tile_stride = (tile_bytes + 1023) & ~1023LL;      // whole 1 KB pieces per wavefront
    float *Lt = reinterpret_cast<float *>(smem_t + yzone + wave * tile_stride);
    {
        const int pieces = (int)((ybytes + 1023) >> 10);
        for (int p = wave; p < pieces; p += 4) {
            long long off = ((long long)p << 10) + lane * 16;
            if (off > ybytes - 16) off = ybytes - 16;                 // (the tail lanes of the last piece repeat its last 16 bytes)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const char *>(Y) + off,
                                             (__attribute__((address_space(3))) void *)(smem_t + ((long long)p << 10)), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // A repeating lane still writes at ITS OWN LDS position (destination = base + 16 * lane).  With N * K / 2 odd the copy ends
        // 8 bytes into a lane's slot: that lane has put bytes [ybytes - 16, ybytes - 8) where the last two floats belong.  They are
        // read again with an ordinary load (nothing is read beyond the operator's end).
        if ((ybytes & 8) && threadIdx.x == 0)
            *reinterpret_cast<float2 *>(Ys + ybytes / 4 - 2) = *reinterpret_cast<const float2 *>(Y + ybytes / 4 - 2);
        // behind the last row of the operator: zeros (the over-read of row N - 1 and the rows N .. of the last column block)
        for (long long pos = ybytes / 4 + threadIdx.x; pos < yzone / 4; pos += blockDim.x) Ys[pos] = 0.0f;
        __syncthreads();
    }
    LPH_ADD(0, t0);
    // the tile of rows m0 .. m0 + 31 -> this wavefront's LDS block (whole 1 KB pieces; the tail lanes of the last piece repeat
    // its last 16 bytes, which land behind the tile's rows -- but for the one lane that straddles their end: process() below)
    auto load_tile = [&](long long m0) {
        const long long rows = (M - m0) < 32 ? (M - m0) : 32;
        const long long bytes = rows * K * 4;
        const char *src = reinterpret_cast<const char *>(L + m0 * K);
        const int pieces = (int)(tile_stride >> 10);
#pragma unroll 4
        for (int p = 0; p < pieces; p++) {
            long long off = ((long long)p << 10) + lane * 16;
            if (off > bytes - 16) off = bytes - 16;
            __builtin_amdgcn_global_load_lds(src + off, (__attribute__((address_space(3))) void *)(reinterpret_cast<char *>(Lt) + ((long long)p << 10)),
                                             16, 0, 0);
        }
    };
    // (measured alternatives, both slower than this plain order: issuing the next tile's loads behind the last block's MFMAs so
    //  that they overlap the stores -- 0.064 instead of 0.053 ms; advancing all column blocks together with one read of the left
    //  operand per K-step -- 0.060 ms: the stores of a block then no longer overlap the MFMAs of the next one)
    auto process = [&](long long m0, int c_begin, int c_end) {
        unsigned long long t1 = LPH_T();
        load_tile(m0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // (also: the previous tile's stores are out)
        // a last tile with an odd number of rows and K / 2 odd ends 8 bytes into a lane's 16-byte slot: as for the operator above, the
        // repeating lane has shifted the last two floats of the last row; an ordinary load puts them right (wavefront-uniform test)
        if (M - m0 < 32 && (((M - m0) * K) & 2)) {
            const long long last = (M - m0) * K - 2;
            if (lane == 0) *reinterpret_cast<float2 *>(Lt + last) = *reinterpret_cast<const float2 *>(L + m0 * K + last);
        }
        LPH_ADD(1, t1);
        const float2 *arow = reinterpret_cast<const float2 *>(Lt + (size_t)l32 * K + 2 * half * KH2);
        for (int c = c_begin; c < c_end; c++) {
            t1 = LPH_T();
            const int n0 = 32 * c;
            const float2 *yrow = reinterpret_cast<const float2 *>(Ys + (size_t)(n0 + l32) * K + 2 * half * KH2);
            floatx16 acc;
#pragma unroll
            for (int i = 0; i < 16; i++) acc[i] = 0.0f;
#pragma unroll
            for (int j = 0; j < KH2; j++) {
                const int k = 2 * half * KH2 + 2 * j;
                float2 a2 = arow[j];
                const float2 b2 = yrow[j];
                if (2 * KH2 + 2 * j >= K) {                          // (compile-time position: only the last columns of the second half)
                    a2.x = (k < K) ? a2.x : 0.0f;
                    a2.y = (k + 1 < K) ? a2.y : 0.0f;
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2.x, b2.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2.y, b2.y, acc, 0, 0, 0);
            }
            LPH_ADD(2, t1); t1 = LPH_T();
            const int n = n0 + l32;
            if (n < N) {
                const int col = idx_out[n];
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const long long r = m0 + 8 * (i / 4) + 4 * half + (i % 4);
                    if (r < M) out[r * nS + col] = acc[i];
                }
            }
            LPH_ADD(3, t1);
        }
#ifdef AMX_LUT_PHASES
        ph[5] += 1;
#endif
    };
    // Whole tiles first, the same number for every wavefront; the tiles that are left over (2250 tiles over 1024 wavefronts: 202)
    // are cut into their column blocks, so that the launch ends after 2 1/3 tiles' worth of work instead of 3.
    const int nb = (N + 31) >> 5;
    const long long T = (M + 31) >> 5, W = (long long)gridDim.x * 4, wid = (long long)blockIdx.x * 4 + wave;
    const long long F = T / W;
    for (long long f = 0; f < F; f++) process((wid + f * W) * 32, 0, nb);
    for (long long u = wid; u < (T - F * W) * nb; u += W) process((F * W + u / nb) * 32, (int)(u % nb), (int)(u % nb) + 1);
#ifdef AMX_LUT_PHASES
    ph[7] = LPH_T() - t_all;
    if (lane == 0) for (int k = 0; k < 8; k++) atomicAdd(&g_lut_ph[k], ph[k]);
#endif
}

// Generic shapes (more than 256 reduction indices, or an SH -> signal operator beyond the LDS: SANDI's 5 shells x 91
// coefficients x 300 volumes): one wavefront = 32 rows of L against 32 columns at a time, operands straight from L2.  The reduction
// index is split in two halves, one per half-wavefront (lane l works on k = (l / 32) * Kh + j), so that every lane
// streams a contiguous piece of its row of L and of its row of Ylm; the order of a sum does not matter to the GEMM.
__global__ __launch_bounds__(256) void k_lut_resample_generic(const float *__restrict__ L, const float *__restrict__ Y,
                                                      const int *__restrict__ idx_out, long long M, int K, int N, int nS,
                                                      float *__restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int Kh = (K + 1) / 2;
    const long long m0 = ((long long)blockIdx.x * 4 + wave) * 32;
    if (m0 >= M) return;
    const long long row = m0 + l32;
    const float *lrow = L + (row < M ? row : M - 1) * K + (long long)half * Kh;
    const int kcnt = half == 0 ? Kh : K - Kh;                        // elements of this lane's half
    for (int n0 = 0; n0 < N; n0 += 32) {
        const int n = n0 + l32;
        const float *yrow = Y + (long long)(n < N ? n : N - 1) * K + (long long)half * Kh;
        floatx16 acc;
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = 0.0f;
        for (int j = 0; j < Kh; j++) {
            const float av = (j < kcnt && row < M) ? lrow[j] : 0.0f;
            const float bv = (j < kcnt && n < N) ? yrow[j] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        if (n < N) {
            const int col = idx_out[n];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const long long r = m0 + 8 * (i / 4) + 4 * half + (i % 4);
                if (r < M) out[r * nS + col] = acc[i];
            }
        }
    }
}

}  // namespace amx

// shared by amx_lut_resample (lm given) and amx_lut_rotate_resample (zonal factors + basis values given): device buffers
// d_lm or (d_z, d_r) -> ctx->hextra (f32 [n_rows][nS], ones outside idx_out)
static int lut_gemm(amx_ctx *ctx, const float *d_lm, const float *d_z, const float *d_r, int ndirs, int n_sh1, int64_t n_rows,
                    int n_sh, const float *d_ylm, const int *d_idx, int n_out, int nS)
{
    int rc = AMX_OK;
    hipLaunchKernelGGL(amx::k_fill_ones, dim3(2048), dim3(256), 0, nullptr, (float *)ctx->hextra.p, (long long)n_rows * nS);
    const amx::LutRoute rt = amx::lut_route(n_sh, n_out, d_lm == nullptr);      // (amx_lut_route.hpp: the one place that decides)
    const int kh2t = rt.kh2;
    const size_t lds = rt.lds;
    if (rt.route == amx::LUT_ROUTE_REFUSED)
        return amx_bad(ctx, "amx_lut_rotate_resample: shape beyond the fused kernel (K <= 256, operator <= 80 KB)");
    if (rt.route == amx::LUT_ROUTE_TILE) {                           // both operands in LDS
        auto launch = [&](auto kern) -> int {
            HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            long long blocks = (n_rows + 127) / 128;
            if (blocks > ctx->n_cu) blocks = ctx->n_cu;              // persistent, one workgroup per CU: the operator is staged once
            rec(ctx, 8, nullptr);
            hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, nullptr, d_lm, d_ylm, d_idx, (long long)n_rows, n_sh,
                               n_out, nS, (float *)ctx->hextra.p);
            return AMX_OK;
        };
        if (kh2t == 23) rc = launch(amx::k_lut_resample_tile<23>);
        else if (kh2t == 46) rc = launch(amx::k_lut_resample_tile<46>);
        else rc = launch(amx::k_lut_resample_tile<64>);
        if (rc) return rc;
    } else if (rt.route == amx::LUT_ROUTE_GENERIC) {                 // operands from L2
        rec(ctx, 8, nullptr);
        hipLaunchKernelGGL(amx::k_lut_resample_generic, dim3((unsigned)((n_rows + 127) / 128)), dim3(256), 0, nullptr, d_lm, d_ylm,
                           d_idx, (long long)n_rows, n_sh, n_out, nS, (float *)ctx->hextra.p);
    } else {
        auto launch = [&](auto kern) -> int {
            HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            long long blocks = (n_rows + 127) / 128;                  // persistent: the Ylm tile is staged once per workgroup
            const long long cap = 2LL * ctx->n_cu;
            if (blocks > cap) blocks = cap;
            rec(ctx, 8, nullptr);
            hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, nullptr, d_lm, d_ylm, d_idx, (long long)n_rows, n_sh,
                               n_out, nS, (float *)ctx->hextra.p, d_z, d_r, ndirs, n_sh1);
            return AMX_OK;
        };
        if (kh2t == 23) rc = launch(amx::k_lut_resample<23>);
        else if (kh2t == 46) rc = launch(amx::k_lut_resample<46>);
        else rc = launch(amx::k_lut_resample<64>);
        if (rc) return rc;
    }
    HIPCHK(ctx, hipGetLastError());
    rec(ctx, 9, nullptr);
    return AMX_OK;
}

extern "C" int amx_lut_route(int n_sh, int n_out, int fused, int64_t out[3])
{
    if (n_sh < 1 || n_out < 1 || !out) return AMX_E_BADARG;
    const amx::LutRoute rt = amx::lut_route(n_sh, n_out, fused != 0);
    out[0] = rt.route; out[1] = rt.kh2; out[2] = (int64_t)rt.lds;
    return AMX_OK;
}

extern "C" int amx_lut_resample(amx_ctx *ctx, const float *lm, int64_t n_rows, int n_sh, const float *ylm_out,
                                const int32_t *idx_out, int n_out, int nS, float *out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!lm || !ylm_out || !idx_out || !out || n_rows < 1 || n_sh < 1 || n_out < 1 || nS < n_out)
        return amx_bad(ctx, "amx_lut_resample: bad argument");
    for (int k = 0; k < n_out; k++) if (idx_out[k] < 0 || idx_out[k] >= nS) return amx_bad(ctx, "amx_lut_resample: idx_out out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t lb = (size_t)n_rows * n_sh * sizeof(float), yb = (size_t)n_out * n_sh * sizeof(float);
    const size_t ob = (size_t)n_rows * nS * sizeof(float);
    if ((rc = amx_ensure(ctx, ctx->hy, lb))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hdirs, yb))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hrmse, (size_t)n_out * sizeof(int)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hextra, ob))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->hy.p, lm, lb, hipMemcpyHostToDevice, nullptr));
    HIPCHK(ctx, hipMemcpyAsync(ctx->hdirs.p, ylm_out, yb, hipMemcpyHostToDevice, nullptr));
    HIPCHK(ctx, hipMemcpyAsync(ctx->hrmse.p, idx_out, (size_t)n_out * sizeof(int), hipMemcpyHostToDevice, nullptr));
    if ((rc = lut_gemm(ctx, (const float *)ctx->hy.p, nullptr, nullptr, 1, 1, n_rows, n_sh, (const float *)ctx->hdirs.p,
                       (const int *)ctx->hrmse.p, n_out, nS))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->hextra.p, ob, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}

extern "C" int amx_lut_rotate_resample(amx_ctx *ctx, const float *zonal, int n_atoms, const float *ylm_rot, int ndirs,
                                       int n_sh_shell, int n_shells, const float *ylm_out, const int32_t *idx_out, int n_out,
                                       int nS, float *out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!zonal || !ylm_rot || !ylm_out || !idx_out || !out || n_atoms < 1 || ndirs < 1 || n_sh_shell < 1 || n_shells < 1 ||
        n_out < 1 || nS < n_out)
        return amx_bad(ctx, "amx_lut_rotate_resample: bad argument");
    for (int k = 0; k < n_out; k++) if (idx_out[k] < 0 || idx_out[k] >= nS) return amx_bad(ctx, "amx_lut_rotate_resample: idx_out out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const int K = n_sh_shell * n_shells;
    const int64_t n_rows = (int64_t)n_atoms * ndirs;
    const size_t zb = (size_t)n_atoms * K * sizeof(float), rb = (size_t)ndirs * n_sh_shell * sizeof(float);
    const size_t yb = (size_t)n_out * K * sizeof(float), ob = (size_t)n_rows * nS * sizeof(float);
    if ((rc = amx_ensure(ctx, ctx->hy, zb + rb + 64))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hdirs, yb))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hrmse, (size_t)n_out * sizeof(int)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hextra, ob))) return rc;
    float *d_z = (float *)ctx->hy.p, *d_r = (float *)((char *)ctx->hy.p + ((zb + 15) & ~(size_t)15));
    HIPCHK(ctx, hipMemcpyAsync(d_z, zonal, zb, hipMemcpyHostToDevice, nullptr));
    HIPCHK(ctx, hipMemcpyAsync(d_r, ylm_rot, rb, hipMemcpyHostToDevice, nullptr));
    HIPCHK(ctx, hipMemcpyAsync(ctx->hdirs.p, ylm_out, yb, hipMemcpyHostToDevice, nullptr));
    HIPCHK(ctx, hipMemcpyAsync(ctx->hrmse.p, idx_out, (size_t)n_out * sizeof(int), hipMemcpyHostToDevice, nullptr));
    if ((rc = lut_gemm(ctx, nullptr, d_z, d_r, ndirs, n_sh_shell, n_rows, K, (const float *)ctx->hdirs.p, (const int *)ctx->hrmse.p,
                       n_out, nS))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->hextra.p, ob, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}

#ifdef AMX_LUT_PHASES
extern "C" int amx_debug_lut_phases(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(amx::g_lut_ph), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(amx::g_lut_ph), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
#endif
