// amx_noise.hip -- the noise level of an image from the spread of its b0 repeats (doEstimateNoise; nothing of the
// reference's: its debias and its robust tensor fit both want a number the user has to find elsewhere).
//   k_noise_b0      one lane per voxel: mean, sample standard deviation (ddof = 1) and their ratio over the k b0 samples
//   k_median_hist   one digit of a radix select on the order-preserving 64-bit key of an fp64 value: LDS histogram, merged into a global one
//   k_median_pick   one workgroup: the digit both middle ranks fall into, the ranks that remain
// Per voxel, fp64, every operation rounded on its own (no fused multiply-add), x_i = (double)S[b0_idx[i]] in b0_idx order:
//     sum = ((x_0 + x_1) + x_2) + ...          m  = sum / k
//     q   = ((x_0-m)*(x_0-m) + (x_1-m)*(x_1-m)) + ...          sd = sqrt(q / (k-1))
//     eligible <=> every x_i finite and m > 0 and sd > 0 and sd finite;   mean = m, sd, ratio = m / sd, or NaN in all three
// so that the numpy restatement (tests/noise_np.py) gives the same bits.  The kernel reads only the k b0 samples of a voxel, twice (the
// second time from cache); consecutive lanes take consecutive voxels along the image's fastest spatial axis, so a planar image is read in
// whole lines, while in a volume-fastest image every sample is a line of its own.
// The median is exact: NaNs never enter a histogram, the first pass counts what is left (c) and both middle ranks (c-1)/2 and c/2 are
// narrowed eleven bits at a time (six passes).  Only integer counts are accumulated, so the result depends on neither the launch shape nor the order
// of the atomics.  Nothing comes back to the host between the passes: the state (prefixes, residual ranks) lives beside the histograms.
#include "amx_host.hpp"

namespace amx {

constexpr int kNoiseMaxB0 = 128;
constexpr int kMedBits = 11, kMedBins = 1 << kMedBits, kMedPasses = (64 + kMedBits - 1) / kMedBits;   // six passes: five of 11 bits, one of 9
constexpr int kMedRing = 4;             // workspace slots: call k of a ctx takes slot k mod kMedRing (calls on different streams)

struct NoiseArgs {
    const void *in;               // float | double samples
    const int *rank;              // [d2][d1][d0]: row of the outputs, -1 = not visited (image form) or null: every voxel, in order
    const int *b0dev;             // the plan's b0 list in device memory, or null: b0[] below
    double *mean, *sd, *ratio;    // [n_vox] each, any may be null
    long long d0, d1, d2, s0, s1, s2, sv;
    int n_b0;
    int b0[kNoiseMaxB0];
};

template <typename T>
__global__ __launch_bounds__(256) void k_noise_b0(NoiseArgs a)
{
#pragma clang fp contract(off)
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.d0 * a.d1 * a.d2) return;
    const long long r = a.rank ? (long long)a.rank[m] : m;
    if (r < 0) return;
    const long long i0 = m % a.d0, i1 = (m / a.d0) % a.d1, i2 = m / (a.d0 * a.d1);
    const T *src = static_cast<const T *>(a.in) + i0 * a.s0 + i1 * a.s1 + i2 * a.s2;
    const int k = a.n_b0;
    double sum = 0.0;
    bool finite = true;
    for (int i = 0; i < k; i++) {
        const double x = (double)src[(long long)(a.b0dev ? a.b0dev[i] : a.b0[i]) * a.sv];
        finite = finite && (fabs(x) < INFINITY);
        sum = i == 0 ? x : sum + x;
    }
    const double mu = sum / (double)k;
    double q = 0.0;
    for (int i = 0; i < k; i++) {
        const double x = (double)src[(long long)(a.b0dev ? a.b0dev[i] : a.b0[i]) * a.sv];
        const double d = x - mu;
        const double dd = d * d;
        q = i == 0 ? dd : q + dd;
    }
    const double sd = sqrt(q / (double)(k - 1));
    const bool ok = finite && mu > 0.0 && sd > 0.0 && sd < INFINITY;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (a.mean) a.mean[r] = ok ? mu : nan;
    if (a.sd) a.sd[r] = ok ? sd : nan;
    if (a.ratio) a.ratio[r] = ok ? mu / sd : nan;
}

// ------------------------------------------------------------------ exact median of the non-NaN values
struct MedState {
    unsigned long long prefix[2];  // the digits settled so far of the lower / upper middle value's key (the rest zero)
    unsigned long long rank[2];    // rank of that value among the values that share its prefix
    unsigned long long count;      // non-NaN values (set by the first pick)
    int same, pad;                 // both prefixes are equal: one histogram serves both
};
constexpr size_t kMedSlotWords = 8 + (size_t)kMedPasses * 2 * kMedBins;       // MedState (64 bytes) + a histogram pair per pass
// pass p settles the bits [med_shift(p), med_shift(p) + med_width(p)) of the key, from the top; the last pass takes what is left
__host__ __device__ constexpr int med_shift(int pass) { return 64 - kMedBits * (pass + 1) > 0 ? 64 - kMedBits * (pass + 1) : 0; }
__host__ __device__ constexpr int med_width(int pass) { return 64 - kMedBits * pass < kMedBits ? 64 - kMedBits * pass : kMedBits; }

// sign bit set -> flip all bits; otherwise flip the sign bit: unsigned order of the keys = numeric order of the values, -0.0 before +0.0
__device__ __forceinline__ unsigned long long med_key(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
}
__device__ __forceinline__ double med_value(unsigned long long key)
{
    const unsigned long long b = (key >> 63) ? (key ^ 0x8000000000000000ull) : ~key;
    return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(256) void k_median_hist(const double *__restrict__ v, long long n, int pass, const MedState *__restrict__ st,
                                                     unsigned long long *__restrict__ hist)
{
    __shared__ unsigned int sh[2 * kMedBins];
    for (int i = threadIdx.x; i < 2 * kMedBins; i += blockDim.x) sh[i] = 0u;
    const unsigned long long p0 = st->prefix[0], p1 = st->prefix[1], cnt = st->count;
    const bool two = pass > 0 && !st->same;
    __syncthreads();
    if (pass > 0 && cnt == 0) return;                     // (the same for every thread: nothing but NaNs, the first pick has answered)
    const int shift = med_shift(pass), above = shift + med_width(pass);          // above < 64 from the second pass on
    const unsigned mask = (1u << med_width(pass)) - 1u;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long base = (long long)blockIdx.x * blockDim.x; base < n; base += step) {
        const long long idx = base + threadIdx.x;
        if (idx < n) {
            const double x = v[idx];
            if (x == x) {
                const unsigned long long key = med_key(x);
                const unsigned d = (unsigned)(key >> shift) & mask;
                if (pass == 0) {
                    atomicAdd(&sh[d], 1u);
                } else {
                    if (((key ^ p0) >> above) == 0) atomicAdd(&sh[d], 1u);
                    if (two && ((key ^ p1) >> above) == 0) atomicAdd(&sh[kMedBins + d], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * kMedBins; i += blockDim.x)
        if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
}

// <<<1, kPickThreads>>>: thread t owns the kMedPer consecutive digits from t * kMedPer
constexpr int kPickThreads = 256, kMedPer = kMedBins / kPickThreads;
static_assert(kMedBins % kPickThreads == 0, "every thread of the pick owns the same number of digits");
__global__ __launch_bounds__(kPickThreads) void k_median_pick(MedState *st, const unsigned long long *__restrict__ hist, int pass,
                                                              double *__restrict__ out, long long *__restrict__ count)
{
    __shared__ unsigned long long sc[2][kPickThreads];
    __shared__ unsigned long long newp[2];
    const int t = threadIdx.x;
    const MedState s = *st;
    if (pass > 0 && s.count == 0) return;
    const bool two = pass > 0 && !s.same;
    unsigned long long h[2][kMedPer], own[2] = {0ull, 0ull};
#pragma unroll
    for (int j = 0; j < kMedPer; j++) {
        h[0][j] = hist[t * kMedPer + j];
        h[1][j] = two ? hist[kMedBins + t * kMedPer + j] : h[0][j];
        own[0] += h[0][j]; own[1] += h[1][j];
    }
    sc[0][t] = own[0]; sc[1][t] = own[1];
    __syncthreads();
    for (int off = 1; off < kPickThreads; off <<= 1) {      // inclusive scan of the threads' sums, both rows
        const unsigned long long a0 = t >= off ? sc[0][t - off] : 0ull, a1 = t >= off ? sc[1][t - off] : 0ull;
        __syncthreads();
        sc[0][t] += a0; sc[1][t] += a1;
        __syncthreads();
    }
    const unsigned long long total = sc[0][kPickThreads - 1];
    if (pass == 0 && total == 0) {                          // n == 0 or nothing but NaNs
        if (t == 0) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            out[0] = nan; out[1] = nan; *count = 0;
        }
        return;
    }
    const unsigned long long r[2] = {pass == 0 ? (total - 1) / 2 : s.rank[0], pass == 0 ? total / 2 : s.rank[1]};
    const int shift = med_shift(pass);
#pragma unroll
    for (int w = 0; w < 2; w++) {
        unsigned long long below = sc[w][t] - own[w];       // values in the digits of the threads before this one
#pragma unroll
        for (int j = 0; j < kMedPer; j++) {
            if (below <= r[w] && r[w] < below + h[w][j]) {  // true for exactly one digit of one thread: the rank is below the total
                newp[w] = s.prefix[w] | ((unsigned long long)(t * kMedPer + j) << shift);
                st->rank[w] = r[w] - below;
            }
            below += h[w][j];
        }
    }
    __syncthreads();
    if (t == 0) {
        st->prefix[0] = newp[0]; st->prefix[1] = newp[1];
        st->same = newp[0] == newp[1];
        if (pass == 0) { st->count = total; *count = (long long)total; }
        if (pass == kMedPasses - 1) { out[0] = med_value(newp[0]); out[1] = med_value(newp[1]); }
    }
}

}  // namespace amx

using namespace amx;

namespace {

int noise_check(amx_ctx *ctx, int nS, const int32_t *b0_idx, int n_b0)
{
    if (nS < 1) return amx_bad(ctx, "amx_noise_b0: bad sizes (need nS >= 1)");
    if (n_b0 < 2) return amx_bad(ctx, "amx_noise_b0: the spread of the b0 repeats needs at least 2 b0 volumes");
    if (n_b0 > kNoiseMaxB0) return amx_bad(ctx, "amx_noise_b0: more than 128 b0 volumes");
    if (b0_idx) for (int i = 0; i < n_b0; i++) if (b0_idx[i] < 0 || b0_idx[i] >= nS) return amx_bad(ctx, "amx_noise_b0: b0 index out of range");
    return AMX_OK;
}

template <typename T>
int noise_launch(amx_ctx *ctx, const NoiseArgs &a, hipStream_t s)
{
    const long long total = a.d0 * a.d1 * a.d2;
    hipLaunchKernelGGL((k_noise_b0<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    HIPCHK(ctx, hipGetLastError());
    amx_note(ctx, "k_noise_b0");
    return AMX_OK;
}

template <typename T>
int noise_rows_dev(amx_ctx *ctx, const T *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double *d_mean, double *d_sd, double *d_ratio,
                   void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (n < 0 || !b0_idx) return amx_bad(ctx, "amx_noise_b0_rows: bad argument");
    int rc;
    if ((rc = noise_check(ctx, nS, b0_idx, n_b0))) return rc;
    if (!d_mean && !d_sd && !d_ratio) return amx_bad(ctx, "amx_noise_b0_rows: no output buffer (give at least one of mean, sd, ratio)");
    if (n == 0) return AMX_OK;
    if (!d_S) return amx_bad(ctx, "amx_noise_b0_rows: null buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    NoiseArgs a;
    memset(&a, 0, sizeof a);
    a.in = d_S; a.mean = d_mean; a.sd = d_sd; a.ratio = d_ratio;
    a.d0 = n; a.d1 = 1; a.d2 = 1; a.s0 = nS; a.sv = 1; a.n_b0 = n_b0;
    for (int i = 0; i < n_b0; i++) a.b0[i] = b0_idx[i];
    return noise_launch<T>(ctx, a, (hipStream_t)hip_stream);
}

}  // namespace

extern "C" {

int amx_noise_b0_rows_device(amx_ctx *ctx, const double *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double *d_mean, double *d_sd,
                             double *d_ratio, void *hip_stream)
{
    return noise_rows_dev<double>(ctx, d_S, n, nS, b0_idx, n_b0, d_mean, d_sd, d_ratio, hip_stream);
}

int amx_noise_b0_rows_device_f32(amx_ctx *ctx, const float *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double *d_mean, double *d_sd,
                                 double *d_ratio, void *hip_stream)
{
    return noise_rows_dev<float>(ctx, d_S, n, nS, b0_idx, n_b0, d_mean, d_sd, d_ratio, hip_stream);
}

int amx_prep_noise_b0_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, double *d_mean, double *d_sd, double *d_ratio, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_noise_b0: not a plan of this ctx");
    int rc;
    if ((rc = noise_check(ctx, p->nS, nullptr, p->n_b0))) return rc;
    if (!d_mean && !d_sd && !d_ratio) return amx_bad(ctx, "amx_prep_noise_b0: no output buffer (give at least one of mean, sd, ratio)");
    if (p->n_vox == 0) return AMX_OK;
    if (!d_img) return amx_bad(ctx, "amx_prep_noise_b0: null buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    NoiseArgs a;
    memset(&a, 0, sizeof a);
    a.in = d_img; a.rank = p->rank; a.b0dev = p->b0idx; a.mean = d_mean; a.sd = d_sd; a.ratio = d_ratio;
    a.d0 = p->d[0]; a.d1 = p->d[1]; a.d2 = p->d[2]; a.s0 = p->s[0]; a.s1 = p->s[1]; a.s2 = p->s[2]; a.sv = p->sv; a.n_b0 = p->n_b0;
    return noise_launch<float>(ctx, a, (hipStream_t)hip_stream);
}

int amx_nanmedian_device(amx_ctx *ctx, const double *d_v, int64_t n, double *d_out, int64_t *d_count, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (n < 0) return amx_bad(ctx, "amx_nanmedian: bad argument (n < 0)");
    if (!d_out || !d_count) return amx_bad(ctx, "amx_nanmedian: null output");
    if (n > 0 && !d_v) return amx_bad(ctx, "amx_nanmedian: null buffer");
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t slot = kMedSlotWords * sizeof(unsigned long long);
    if ((rc = amx_ensure(ctx, ctx->median_ws, slot * kMedRing))) return rc;
    unsigned long long *ws = (unsigned long long *)ctx->median_ws.p + (size_t)(ctx->median_seq++ % kMedRing) * kMedSlotWords;
    MedState *st = reinterpret_cast<MedState *>(ws);
    static_assert(sizeof(MedState) <= 8 * sizeof(unsigned long long), "MedState fills the first eight words of a slot");
    HIPCHK(ctx, hipMemsetAsync(ws, 0, slot, s));
    // a lane takes four values or more; at most four workgroups per compute unit (each merges its non-empty bins into the global histogram)
    long long grid = (n + 1023) / 1024;
    const long long cap = (long long)ctx->n_cu * 4;
    grid = grid < 1 ? 1 : (grid > cap ? cap : grid);
    for (int pass = 0; pass < kMedPasses; pass++) {
        unsigned long long *hist = ws + 8 + (size_t)pass * 2 * kMedBins;
        hipLaunchKernelGGL(k_median_hist, dim3((unsigned)grid), dim3(256), 0, s, d_v, (long long)n, pass, st, hist);
        hipLaunchKernelGGL(k_median_pick, dim3(1), dim3(kPickThreads), 0, s, st, hist, pass, d_out, (long long *)d_count);
    }
    HIPCHK(ctx, hipGetLastError());
    amx_note(ctx, "k_median_hist");
    amx_note(ctx, "k_median_pick");
    return AMX_OK;
}

}  // extern "C"
