// amx_debias.hip -- Rician debias of the raw signal (doDebiasSignal / DWI-SNR): core.py:201-206 -> preproc.py:23-36 debiasRician.
// Per masked voxel the reference takes sigma = mean(S[b0_idx]) / SNR and minimises over E, from E = S, with scipy's L-BFGS-B
//     F(E) = sum_i (S_i - mu(E_i))^2,   mu(e) = sigma sqrt(pi/2) L_{1/2}(-e^2 / (2 sigma^2))      (preproc.py:8-12)
// mu(e) is the mean of a Rician variable of underlying amplitude e.  F is separable; mu is increasing and convex on e >= 0 with
// mu(0) = |sigma| sqrt(pi/2) (the noise floor) and mu(e) > e.  The minimiser is therefore E_i = mu^-1(S_i) above the floor and
// E_i = 0 at or below it -- which is what the kernels here compute, sample by sample in fp64 (the reference's quasi-Newton run stops
// on its relative-reduction test some 1e-5 .. 1e-3 b0 short of it: DESIGN.md).  Only sigma^2 enters.
//
//   k_debias_sigma   one lane per voxel: the b0 mean in the samples' precision and numpy's summation order
//                    (`DWI[ix,iy,iz,scheme.b0_idx].mean()`, preproc.py:30: eight running sums, combined pairwise), / SNR in fp64
//   k_debias         one lane per sample, walking the image in memory order: floor test, root of mu(e) = S by Newton's method
//
// In units of sigma (t = e / |sigma|, s = S / |sigma|, x = t^2 / 2):
//     m(t)  = sqrt(pi/2) [(1 + x) I0e(x/2) + x I1e(x/2)]          m'(t) = sqrt(pi/2) (t/2) [I0e(x/2) + I1e(x/2)]
// and for x > 1e4, where the closed form is no better than its series,  m(t) = t + 1/(2t) + 1/(8t^3) + 3/(16t^5).
// m(t) - s is convex and increasing, so Newton's iterates descend to the root from any point right of it and reach such a point in one
// step from any point left of it.  Start: t = 2 sqrt(s / m(0) - 1), the root of the small-t form m(0) (1 + t^2/4) >= m(t) (a lower
// bound of the root, exact as s -> floor, where m' vanishes and Newton from E = S would crawl), or s - 1/(2s) for s > 3; every iterate
// is kept in [that lower bound, s].  A numpy run of the same arithmetic needed at most 5 evaluations on 500 000 values of s in
// (floor, 1e7] (a CPU trial, not a tested bound: the tests pin that no sample reaches the cap); the loop runs until every lane of the
// wavefront is done, kDebiasTrips at most, and a sample that reaches the cap is counted (amx_debias_last_unconverged).
// I0e / I1e: Chebyshev series in z/4 - 1 on [0, 8] and in 16/z - 1 (times 1/sqrt z) beyond, relative error <= 1.6e-15; the coefficients
// are made by tools/gen_debias_cheb.py.
#include "amx_host.hpp"
#include <cmath>

namespace amx {

__constant__ double kA0[30] = {
    0.6767952744094761, -0.3046826723431984, 0.17162090152220877,
    -0.09490109704804764, 0.04930528423967071, -0.02373741480589947,
    0.010546460394594998, -0.004324309995050576, 0.0016394756169413357,
    -0.0005763755745385824, 0.00018850288509584165, -5.754195010082104e-05,
    1.6448448070728896e-05, -4.4167383584587505e-06, 1.1173875391201037e-06,
    -2.670793853940612e-07, 6.046995022541919e-08, -1.300025009986248e-08,
    2.6598237246823866e-09, -5.189795601635263e-10, 9.675809035373237e-11,
    -1.726826291441556e-11, 2.95505266312964e-12, -4.856446783111929e-13,
    7.676185498604936e-14, -1.1685332877993451e-14, 1.715391285555133e-15,
    -2.431279846547955e-16, 3.3307945188222384e-17, -4.4153416464793395e-18,
};
__constant__ double kA1[30] = {
    0.25258718644363365, -0.17641651835783406, 0.1026436586898471,
    -0.05294598120809499, 0.024726449030626516, -0.010564084894626197,
    0.004156422944312888, -0.0015135724506312532, 0.0005122859561685758,
    -0.00016176081582589674, 4.781565107550054e-05, -1.3273163656039436e-05,
    3.4702513081376785e-06, -8.568720264695455e-07, 2.0032947535521353e-07,
    -4.445059128796328e-08, 9.381537386495773e-09, -1.8872497517228294e-09,
    3.625590281552117e-10, -6.663489723502027e-11, 1.1736186298890901e-11,
    -1.9839743977649436e-12, 3.223793365945575e-13, -5.042185504727912e-14,
    7.600684294735408e-15, -1.1055969477353862e-15, 1.5536319577362005e-16,
    -2.111421214358166e-17, 2.7779141127610464e-18, 0.0,
};
__constant__ double kB0[25] = {
    0.8044904110141088, 0.0033691164782556943, 6.889758346916825e-05,
    2.8913705208347567e-06, 2.0489185894690638e-07, 2.266668990498178e-08,
    3.3962320257083865e-09, 4.94060238822497e-10, 1.1889147107846439e-11,
    -3.1499165279632416e-11, -1.3215811840447713e-11, -1.7941785315068062e-12,
    7.180124451383666e-13, 3.8527783827421426e-13, 1.54008621752141e-14,
    -4.150569347287222e-14, -9.554846698828307e-15, 3.8116806693526224e-15,
    1.7725601330565263e-15, -3.425485619677219e-16, -2.8276239805165836e-16,
    3.461222867697461e-17, 4.46562142029676e-17, -4.830504485944182e-18,
    -7.233180487874754e-18,
};
__constant__ double kB1[25] = {
    0.7785762350182801, -0.009761097491361469, -0.00011058893876262371,
    -3.882564808877691e-06, -2.512236237870209e-07, -2.6314688468895196e-08,
    -3.835380385964237e-09, -5.589743462196584e-10, -1.8974958123505413e-11,
    3.2526035830154884e-11, 1.4125807436613782e-11, 2.0356285441470896e-12,
    -7.198551776245908e-13, -4.0835511110921974e-13, -2.1015418427726643e-14,
    4.272440016711951e-14, 1.0420276984128802e-14, -3.8144030724370075e-15,
    -1.8803547755107825e-15, 3.3082023109209285e-16, 2.96262899764595e-16,
    -3.209525921993424e-17, -4.6503053684893586e-17, 4.414348323071708e-18,
    7.517296310842105e-18,
};

constexpr int kDebiasTrips = 32;            // hard cap of the Newton loop (a CPU trial of the same arithmetic needed 5 evaluations at most)
constexpr int kDebiasMaxB0 = 128;           // b0 volumes k_debias_sigma sums in numpy's order (its block size; beyond it numpy splits recursively)
constexpr double kSqrtHalfPi = 1.2533141373155001;   // float64(sqrt(pi / 2))

struct DebiasArgs {
    const void *in;               // float | double samples
    void *out;                    // float (the image, in place) | double (rows)
    const unsigned char *mask;    // [d2][d1][d0] != 0 selects (image form) or null: every voxel
    double *sigma;                // [d2][d1][d0]
    const int *b0idx;
    unsigned long long *stats;    // samples that reached kDebiasTrips
    long long d0, d1, d2, s0, s1, s2, sv;
    double snr;
    int nS, n_b0, vol_inner;      // vol_inner: the volume axis is the fastest one in memory
};

// sum' c_k T_k(y) of two series at once (Clenshaw)
template <int N>
__device__ __forceinline__ void cheb_pair(const double *__restrict__ c0, const double *__restrict__ c1, double y, double &r0, double &r1)
{
    const double y2 = y + y;
    double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = N - 1; k >= 1; k--) {
        const double ta = fma(y2, a1, c0[k]) - a2, tb = fma(y2, b1, c1[k]) - b2;
        a2 = a1; a1 = ta; b2 = b1; b1 = tb;
    }
    r0 = fma(y, a1, 0.5 * c0[0]) - a2;
    r1 = fma(y, b1, 0.5 * c1[0]) - b2;
}

// m(t) and m'(t), t > 0
__device__ __forceinline__ void rice_mean(double t, double &m, double &dm)
{
    const double x = 0.5 * t * t;
    if (x > 1e4) {
        const double u = 1.0 / (t * t);
        m = t * fma(u, fma(u, fma(u, 0.1875, 0.125), 0.5), 1.0);
        dm = 1.0 - u * fma(u, fma(u, 0.9375, 0.375), 0.5);
        return;
    }
    const double z = 0.5 * x;
    double i0, i1;
    if (z <= 8.0) {
        cheb_pair<30>(kA0, kA1, fma(z, 0.25, -1.0), i0, i1);
        i1 *= z;
    } else {
        cheb_pair<25>(kB0, kB1, 16.0 / z - 1.0, i0, i1);
        const double rs = 1.0 / sqrt(z);
        i0 *= rs; i1 *= rs;
    }
    m = kSqrtHalfPi * fma(x, i0 + i1, i0);
    dm = kSqrtHalfPi * 0.5 * t * (i0 + i1);
}

// numpy's mean of n <= kDebiasMaxB0 values a[idx[i] * stride] in their own precision (umath's pairwise sum below its block size)
template <typename T>
__device__ __forceinline__ T numpy_mean(const T *a, long long stride, const int *__restrict__ idx, int n)
{
    T res;
    if (n < 8) {
        res = (T)0;
        for (int i = 0; i < n; i++) res = res + a[(long long)idx[i] * stride];
    } else {
        T r[8];
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = a[(long long)idx[j] * stride];
        int i = 8;
        for (; i < n - (n % 8); i += 8) {
#pragma unroll
            for (int j = 0; j < 8; j++) r[j] = r[j] + a[(long long)idx[i + j] * stride];
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res = res + a[(long long)idx[i] * stride];
    }
    return res / (T)n;
}

template <typename TIN>
__global__ __launch_bounds__(256) void k_debias_sigma(DebiasArgs a)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.d0 * a.d1 * a.d2) return;
    if (a.mask && !a.mask[m]) return;
    const long long i0 = m % a.d0, i1 = (m / a.d0) % a.d1, i2 = m / (a.d0 * a.d1);
    const TIN *src = static_cast<const TIN *>(a.in) + i0 * a.s0 + i1 * a.s1 + i2 * a.s2;
    a.sigma[m] = (double)numpy_mean<TIN>(src, a.sv, a.b0idx, a.n_b0) / a.snr;
}

template <typename TIN, typename TOUT>
__global__ __launch_bounds__(256) void k_debias(DebiasArgs a)
{
    const long long nvox = a.d0 * a.d1 * a.d2, total = nvox * a.nS;
    const TIN *in = static_cast<const TIN *>(a.in);
    TOUT *out = static_cast<TOUT *>(a.out);
    for (long long base = (long long)blockIdx.x * blockDim.x; base < total; base += (long long)gridDim.x * blockDim.x) {
        const long long idx = base + threadIdx.x;
        const bool live = idx < total;
        long long off = 0;
        double S = 0.0, t = 0.0, tlo = 0.0, s = 0.0, sg = 0.0;
        bool active = false;
        if (live) {
            const long long m = a.vol_inner ? idx / a.nS : idx % nvox, v = a.vol_inner ? idx % a.nS : idx / nvox;
            const long long i0 = m % a.d0, i1 = (m / a.d0) % a.d1, i2 = m / (a.d0 * a.d1);
            off = i0 * a.s0 + i1 * a.s1 + i2 * a.s2 + v * a.sv;
            if (a.mask && !a.mask[m]) {
                out[off] = (TOUT)0;                                   // debiased_DWI = np.zeros(...), preproc.py:24
            } else {
                S = (double)in[off];
                sg = fabs(a.sigma[m]);
                const double fl = sg * kSqrtHalfPi;
                if (!(sg > 0.0) || !(fl < INFINITY) || S != S) {
                    out[off] = (TOUT)S;                               // sigma = 0 (or not finite): F is NaN for every E, nothing is defined
                } else if (!(S > fl)) {
                    out[off] = (TOUT)0;                               // at or below the noise floor: F decreases towards E = 0
                } else {
                    s = S / sg;
                    tlo = 2.0 * sqrt((S - fl) / fl);
                    t = s > 3.0 ? fmax(s - 0.5 / s, tlo) : tlo;
                    t = fmin(t, s);
                    active = true;
                }
            }
        }
        const bool solve = active;
        for (int trip = 0; trip < kDebiasTrips && __any(active); trip++) {
            if (active) {
                double m_, dm;
                rice_mean(t, m_, dm);
                const double h = m_ - s;
                if (fabs(h) <= 16.0 * 2.220446049250313e-16 * s) {
                    active = false;
                } else {
                    const double tn = fmin(fmax(t - h / dm, tlo), s);
                    if (fabs(tn - t) <= 4.440892098500626e-16 * t) active = false;
                    t = tn;
                }
            }
        }
        if (solve) {
            if (active) atomicAdd(a.stats, 1ull);
            out[off] = (TOUT)fmin(t * sg, S);
        }
    }
}

}  // namespace amx

using namespace amx;

namespace {

int debias_check(amx_ctx *ctx, int nS, const int32_t *b0_idx, int n_b0, double snr)
{
    if (nS < 1 || n_b0 < 0 || n_b0 > nS) return amx_bad(ctx, "amx_debias: bad sizes (need 1 <= n_b0 <= nS)");
    if (n_b0 == 0) return amx_bad(ctx, "amx_debias: no b0 volume to estimate the noise level from");
    if (n_b0 > kDebiasMaxB0) return amx_bad(ctx, "amx_debias: more than 128 b0 volumes");
    if (b0_idx) for (int i = 0; i < n_b0; i++) if (b0_idx[i] < 0 || b0_idx[i] >= nS) return amx_bad(ctx, "amx_debias: b0 index out of range");
    if (!(std::isfinite(snr) && snr != 0.0)) return amx_bad(ctx, "amx_debias: the SNR must be finite and not zero");
    return AMX_OK;
}

template <typename TIN, typename TOUT>
int debias_launch(amx_ctx *ctx, DebiasArgs &a, hipStream_t s)
{
    if (!ctx->debias_stats) HIPCHK(ctx, hipMalloc((void **)&ctx->debias_stats, sizeof(unsigned long long)));
    if (!ctx->debias_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->debias_ev, hipEventDisableTiming));
    const long long nvox = a.d0 * a.d1 * a.d2, total = nvox * a.nS;
    int rc;
    if ((rc = amx_ensure(ctx, ctx->debias_sigma, (size_t)nvox * sizeof(double)))) return rc;
    a.sigma = (double *)ctx->debias_sigma.p;
    a.stats = ctx->debias_stats;
    HIPCHK(ctx, hipMemsetAsync(ctx->debias_stats, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL((k_debias_sigma<TIN>), dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, s, a);
    HIPCHK(ctx, hipGetLastError());
    long long grid = (total + 255) / 256;
    const long long cap = (long long)ctx->n_cu * 32;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL((k_debias<TIN, TOUT>), dim3((unsigned)grid), dim3(256), 0, s, a);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->debias_ev, s));      // amx_debias_last_unconverged waits for this, not for the caller's stream
    amx_note(ctx, "k_debias");
    return AMX_OK;
}

template <typename T>
int debias_rows_dev(amx_ctx *ctx, const T *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr, double *d_E, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (n < 0 || !b0_idx) return amx_bad(ctx, "amx_debias_rows: bad argument");
    int rc;
    if ((rc = debias_check(ctx, nS, b0_idx, n_b0, snr))) return rc;
    if (n == 0) return AMX_OK;
    if (!d_S || !d_E) return amx_bad(ctx, "amx_debias_rows: null buffer");
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = amx_ensure(ctx, ctx->debias_b0, (size_t)n_b0 * sizeof(int)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->debias_b0.p, b0_idx, (size_t)n_b0 * sizeof(int), hipMemcpyHostToDevice, s));
    DebiasArgs a;
    memset(&a, 0, sizeof a);
    a.in = d_S; a.out = d_E; a.mask = nullptr; a.b0idx = (const int *)ctx->debias_b0.p;
    a.d0 = n; a.d1 = 1; a.d2 = 1; a.s0 = nS; a.s1 = 0; a.s2 = 0; a.sv = 1;
    a.snr = snr; a.nS = nS; a.n_b0 = n_b0; a.vol_inner = 1;
    return debias_launch<T, double>(ctx, a, s);
}

template <typename T>
int debias_rows_host(amx_ctx *ctx, const T *S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr, double *out_E)
{
    if (!ctx) return AMX_E_BADARG;
    if (n < 0 || !b0_idx) return amx_bad(ctx, "amx_debias_rows: bad argument");
    int rc;
    if ((rc = debias_check(ctx, nS, b0_idx, n_b0, snr))) return rc;
    if (n == 0) return AMX_OK;
    if (!S || !out_E) return amx_bad(ctx, "amx_debias_rows: null buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t cnt = (size_t)n * nS;
    if ((rc = amx_ensure(ctx, ctx->hextra, cnt * sizeof(T)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->hy, cnt * sizeof(double)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->hextra.p, S, cnt * sizeof(T), hipMemcpyHostToDevice, nullptr));
    if ((rc = debias_rows_dev<T>(ctx, (const T *)ctx->hextra.p, n, nS, b0_idx, n_b0, snr, (double *)ctx->hy.p, nullptr))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_E, ctx->hy.p, cnt * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}

}  // namespace

extern "C" {

int amx_debias_rows_device(amx_ctx *ctx, const double *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr,
                           double *d_E, void *hip_stream)
{
    return debias_rows_dev<double>(ctx, d_S, n, nS, b0_idx, n_b0, snr, d_E, hip_stream);
}

int amx_debias_rows_device_f32(amx_ctx *ctx, const float *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr,
                               double *d_E, void *hip_stream)
{
    return debias_rows_dev<float>(ctx, d_S, n, nS, b0_idx, n_b0, snr, d_E, hip_stream);
}

int amx_debias_rows(amx_ctx *ctx, const double *S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr, double *out_E)
{
    return debias_rows_host<double>(ctx, S, n, nS, b0_idx, n_b0, snr, out_E);
}

int amx_debias_rows_f32(amx_ctx *ctx, const float *S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr, double *out_E)
{
    return debias_rows_host<float>(ctx, S, n, nS, b0_idx, n_b0, snr, out_E);
}

// mask u8[X][Y][Z] (host, C order) as given to load_data: debiasRician tests `if mask[ix,iy,iz]` (preproc.py:29), i.e. != 0, where
// the fit gathers mask == 1 (core.py:451) -- the plan keeps both
int amx_prep_set_debias_mask(amx_ctx *ctx, amx_prep *p, const uint8_t *mask)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_set_debias_mask: not a plan of this ctx");
    if (!mask) return amx_bad(ctx, "amx_prep_set_debias_mask: null mask");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned char> mm((size_t)p->n_total);
    for (long long i2 = 0; i2 < p->d[2]; i2++)
        for (long long i1 = 0; i1 < p->d[1]; i1++)
            for (long long i0 = 0; i0 < p->d[0]; i0++)
                mm[(size_t)((i2 * p->d[1] + i1) * p->d[0] + i0)] = mask[i0 * p->c[0] + i1 * p->c[1] + i2 * p->c[2]] != 0;
    if (!p->dmask) HIPCHK(ctx, hipMalloc((void **)&p->dmask, mm.size()));
    HIPCHK(ctx, hipMemcpy(p->dmask, mm.data(), mm.size(), hipMemcpyHostToDevice));
    return AMX_OK;
}

int amx_prep_debias_device(amx_ctx *ctx, const amx_prep *p, float *d_img, double snr, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_debias: not a plan of this ctx");
    int rc;
    if ((rc = debias_check(ctx, p->nS, nullptr, p->n_b0, snr))) return rc;
    if (!p->dmask) return amx_bad(ctx, "amx_prep_debias: the plan has no mask (amx_prep_set_debias_mask)");
    if (!d_img) return amx_bad(ctx, "amx_prep_debias: null buffer");
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DebiasArgs a;
    memset(&a, 0, sizeof a);
    a.in = d_img; a.out = d_img; a.mask = p->dmask; a.b0idx = p->b0idx;
    a.d0 = p->d[0]; a.d1 = p->d[1]; a.d2 = p->d[2]; a.s0 = p->s[0]; a.s1 = p->s[1]; a.s2 = p->s[2]; a.sv = p->sv;
    a.snr = snr; a.nS = p->nS; a.n_b0 = p->n_b0; a.vol_inner = p->sv < p->s[0] ? 1 : 0;
    return debias_launch<float, float>(ctx, a, s);
}

int amx_prep_debias(amx_ctx *ctx, const amx_prep *p, float *img, double snr)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_debias: not a plan of this ctx");
    if (!img) return amx_bad(ctx, "amx_prep_debias: null buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t ib = (size_t)p->extent * sizeof(float);
    if ((rc = amx_ensure(ctx, ctx->hextra, ib))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->hextra.p, img, ib, hipMemcpyHostToDevice, nullptr));
    if ((rc = amx_prep_debias_device(ctx, p, (float *)ctx->hextra.p, snr, nullptr))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(img, ctx->hextra.p, ib, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}

int amx_debias_last_unconverged(amx_ctx *ctx, int64_t *out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!out) return amx_bad(ctx, "amx_debias_last_unconverged: null output");
    *out = 0;
    if (!ctx->debias_stats) return AMX_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize(ctx->debias_ev));
    unsigned long long st = 0;
    HIPCHK(ctx, hipMemcpy(&st, ctx->debias_stats, sizeof st, hipMemcpyDeviceToHost));
    *out = (int64_t)st;
    return AMX_OK;
}

}  // extern "C"
