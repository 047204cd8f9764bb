// amx_unring.hip -- Gibbs ringing removed from every slice of the image by local sub-voxel shifts (doUnring; Kellner et al.,
// MRM 2016; nothing of the reference's).  include/amico_amd.h fixes the arithmetic; tests/unring_np.py restates it.
// A call walks the slices in chunks of UnringRoute::chunk; per chunk, all in float64 scratch [slice][a][b]:
//   k_unring_gather   the chunk's float32 samples, widened; a sample that is not finite flags its slice and is counted once
//   k_unring_dft x 4  the filter Ix = Re IDFT2(DFT2(I) Gx): a one-dimensional complex DFT of 16 lines per workgroup as a product with the
//                     cosine and sine tables on the fp64 matrix cores (v_mfma_f64_16x16x4_f64) -- forward along b, forward along a (and
//                     times Gx), inverse along a, inverse along b (real part, scaled)
//   k_unring_shift x 2  the map U along a of Ix, then U along b of Iy = I - Ix added to it: a workgroup stages 16 lines, walks the 41 shifts,
//                     forms each shifted copy g_j = C_j f in LDS on the matrix cores (the circulant C_j is read from one row d_j of the
//                     shift table), and keeps per pixel the smallest window variation so far and the value it gives; the copies are never stored
//   k_unring_scatter  float32 of the sum into d_out, in the image's layout; a flagged slice gets the image's own bits
// The tables (k_unring_tables) are made per call in float64, every cosine from an integer reduced modulo its period.  Nothing depends on the
// layout, the axes' positions or the chunk: the bits of a slice's result are a function of its samples and (n_a, n_b) alone.  No threshold
// is absolute: the result of 2^k img is 2^k times that of img.  Every loop is a counted loop.
#include "amx_host.hpp"
#include "amx_unring_route.hpp"

namespace amx {

typedef double ur_v4d __attribute__((ext_vector_type(4)));

// C[k][x] = cos(2 pi k x / n), S[k][x] = sin(2 pi k x / n) (both symmetric), D[j][t] = d_j[t] (row 0, the identity, is never read)
__global__ __launch_bounds__(256) void k_unring_tables(double *__restrict__ C, double *__restrict__ S, double *__restrict__ D, int n)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n * n) {
        const int k = e / n, x = e - k * n, m = (k * x) % n;
        const double arg = 2.0 * (double)m / (double)n;
        C[e] = cospi(arg); S[e] = sinpi(arg);
        return;
    }
    const int e2 = e - n * n;
    if (e2 >= kUnringShifts * n) return;
    const int j = e2 / n, t = e2 - j * n;
    if (j == 0) { D[e2] = t == 0 ? 1.0 : 0.0; return; }
    // s_j = jj / 40: cos(2 pi kappa (t + s_j) / n) = cos(2 pi (kappa (40 t + jj) mod 40 n) / (40 n)), all integers
    const int jj = j <= 20 ? j : -(j - 20), P = 40 * n;
    const int q = ((40 * t + jj) % P + P) % P;
    const int K = (n - 1) / 2;                                   // the Nyquist term of an even n is left out
    double acc = 0.0;
    for (int kap = 1; kap <= K; kap++) acc += cospi((double)((kap * q) % P) / (20.0 * (double)n));
    D[e2] = (1.0 + 2.0 * acc) / (double)n;
}

struct UnringGeo {
    long long sa, sb, sc, sv;     // element strides of the two in-plane axes, the third spatial axis and the volumes
    int na, nb, nS;
    int order;                    // which index the threads walk fastest: 0 b, 1 a, 2 the slice (the one with the smallest stride)
};

// element e of a chunk of S slices -> (slice s, ia, ib)
__device__ __forceinline__ void ur_decode(const UnringGeo &g, long long e, int S, int &s, int &ia, int &ib)
{
    if (g.order == 2) { s = (int)(e % S); const long long p = e / S; ib = (int)(p % g.nb); ia = (int)(p / g.nb); }
    else if (g.order == 1) { ia = (int)(e % g.na); const long long p = e / g.na; ib = (int)(p % g.nb); s = (int)(p / g.nb); }
    else { ib = (int)(e % g.nb); const long long p = e / g.nb; ia = (int)(p % g.na); s = (int)(p / g.na); }
}

__device__ __forceinline__ long long ur_offset(const UnringGeo &g, long long sid, int ia, int ib)
{
    const long long z = sid / g.nS, v = sid - z * g.nS;
    return (long long)ia * g.sa + (long long)ib * g.sb + z * g.sc + v * g.sv;
}

__global__ __launch_bounds__(256) void k_unring_gather(const float *__restrict__ img, double *__restrict__ W, int *__restrict__ flags,
                                                       unsigned long long *__restrict__ counter, UnringGeo g, long long slice0, int S)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)S * g.na * g.nb) return;
    int s, ia, ib;
    ur_decode(g, e, S, s, ia, ib);
    const float x = img[ur_offset(g, slice0 + s, ia, ib)];
    W[((size_t)s * g.na + ia) * g.nb + ib] = (double)x;
    if (!isfinite(x) && atomicExch(&flags[s], 1) == 0) atomicAdd(counter, 1ull);
}

__global__ __launch_bounds__(256) void k_unring_scatter(const float *__restrict__ img, const double *__restrict__ T, const int *__restrict__ flags,
                                                        float *__restrict__ out, UnringGeo g, long long slice0, int S)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)S * g.na * g.nb) return;
    int s, ia, ib;
    ur_decode(g, e, S, s, ia, ib);
    const long long off = ur_offset(g, slice0 + s, ia, ib);
    out[off] = flags[s] ? img[off] : (float)T[((size_t)s * g.na + ia) * g.nb + ib];
}

// a batch of lines of one slice: line l, element x at base + l * ls + x * es of a plane
struct UnringLines {
    int n, n_lines, groups;       // line length, lines of a slice, workgroups of a slice
    long long es, ls, plane;
};

// lines (l0 .. l0 + 15) -> F[x][l], rows n .. pad - 1 and lines past the slice's last are zero; sub: the value is sub - src
__device__ __forceinline__ void ur_stage(double *__restrict__ F, const double *__restrict__ src, const double *__restrict__ sub,
                                         const UnringLines &L, size_t base, int l0, int pad)
{
    for (int e = threadIdx.x; e < pad * kUnringLines; e += kUnringThreads) {
        int x, l;
        if (L.es == 1) { x = e % pad; l = e / pad; } else { l = e % kUnringLines; x = e / kUnringLines; }
        double v = 0.0;
        if (x < L.n && l0 + l < L.n_lines) {
            const size_t at = base + (size_t)(l0 + l) * L.ls + (size_t)x * L.es;
            v = sub ? sub[at] - src[at] : src[at];
        }
        F[x * kUnringLd + l] = v;
    }
}

struct UnringDftArgs {
    const double *in_r, *in_i;    // in_i null: a real input
    double *out_r, *out_i;        // out_i null: the real part alone
    const double *C, *S;          // this axis' tables [n][n]
    const double *C_other;        // mode 1: the other axis' cosine table [n_other][n_other]
    int n_other;
    double sg;                    // +1 forward (C - iS), -1 inverse (C + iS)
    int mode;                     // 0 as it is, 1 times Gx (the lines' index is k_b, the output's k_a), 2 times scale
    double scale;
    UnringLines L;
};

__global__ __launch_bounds__(kUnringThreads) void k_unring_dft(UnringDftArgs a)
{
    extern __shared__ double ur_lds[];
    const UnringLines &L = a.L;
    const int n = L.n, pad = (n + kUnringTile - 1) / kUnringTile * kUnringTile;
    double *Fr = ur_lds, *Fi = ur_lds + (size_t)pad * kUnringLd;
    const int s = blockIdx.x / L.groups, l0 = (blockIdx.x - s * L.groups) * kUnringLines;
    const size_t base = (size_t)s * L.plane;
    ur_stage(Fr, a.in_r, nullptr, L, base, l0, pad);
    if (a.in_i) ur_stage(Fi, a.in_i, nullptr, L, base, l0, pad);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, h = lane >> 4;
    for (int m = wave; m < pad / kUnringTile; m += kUnringThreads / 64) {
        ur_v4d acc_r = {0.0, 0.0, 0.0, 0.0}, acc_i = {0.0, 0.0, 0.0, 0.0};
        const int col = kUnringTile * m + c;                     // the output index this lane's A row stands for (the tables are symmetric)
        for (int ks = 0; ks < pad / kUnringK; ks++) {
            const int xk = kUnringK * ks + h;
            const bool in = col < n && xk < n;
            const double cv = in ? a.C[(size_t)xk * n + col] : 0.0, sv = in ? a.sg * a.S[(size_t)xk * n + col] : 0.0;
            const double fr = Fr[xk * kUnringLd + c];
            acc_r = __builtin_amdgcn_mfma_f64_16x16x4f64(cv, fr, acc_r, 0, 0, 0);
            if (a.out_i) acc_i = __builtin_amdgcn_mfma_f64_16x16x4f64(-sv, fr, acc_i, 0, 0, 0);
            if (a.in_i) {
                const double fi = Fi[xk * kUnringLd + c];
                acc_r = __builtin_amdgcn_mfma_f64_16x16x4f64(sv, fi, acc_r, 0, 0, 0);
                if (a.out_i) acc_i = __builtin_amdgcn_mfma_f64_16x16x4f64(cv, fi, acc_i, 0, 0, 0);
            }
        }
        const int l = l0 + c;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int k = kUnringTile * m + h + 4 * g;
            if (k < n && l < L.n_lines) {
                double f = 1.0;
                if (a.mode == 1) {
                    // a_n(k) = 1 + cos(2 pi k / n); Gx = a_nb(kb) / (a_na(ka) + a_nb(kb)), 1/2 where both vanish (both axes at Nyquist)
                    const double aa = 1.0 + a.C[(size_t)k * n + 1], ab = 1.0 + a.C_other[(size_t)l * a.n_other + 1], den = aa + ab;
                    f = den == 0.0 ? 0.5 : ab / den;
                } else if (a.mode == 2) f = a.scale;
                const size_t at = base + (size_t)l * L.ls + (size_t)k * L.es;
                a.out_r[at] = acc_r[g] * f;
                if (a.out_i) a.out_i[at] = acc_i[g] * f;
            }
        }
    }
}

struct UnringShiftArgs {
    const double *src, *sub;      // the line's value is src, or sub - src where sub is given
    const double *add;            // null, or what the result is added to (same index as dst; may be dst)
    double *dst;
    const double *D;              // [41][n]
    UnringLines L;
};

// one shift's candidates for the pixels of this thread: TV of the three differences left and right of the pixel in G, the first strict
// minimum so far wins; val is the interpolated value the winner gives
template <int NPIX>
__device__ __forceinline__ void ur_windows(const double *__restrict__ G, int n, int xq, int l, double s, double (&best)[NPIX], double (&val)[NPIX])
{
#pragma unroll
    for (int i = 0; i < NPIX; i++) {
        const int x = xq + 16 * i;
        if (x < n) {
            double g[9];
#pragma unroll
            for (int o = 0; o < 9; o++) {
                int xm = x + o - 4;
                xm = xm < 0 ? xm + n : (xm >= n ? xm - n : xm);
                g[o] = G[xm * kUnringLd + l];
            }
            const double tvl = fabs(g[3] - g[2]) + fabs(g[2] - g[1]) + fabs(g[1] - g[0]);
            const double tvr = fabs(g[5] - g[6]) + fabs(g[6] - g[7]) + fabs(g[7] - g[8]);
            const double cand = s > 0.0 ? (1.0 - s) * g[4] + s * g[3] : (1.0 + s) * g[4] - s * g[5];
            if (tvl < best[i]) { best[i] = tvl; val[i] = cand; }
            if (tvr < best[i]) { best[i] = tvr; val[i] = cand; }
        }
    }
}

__global__ __launch_bounds__(kUnringThreads) void k_unring_shift(UnringShiftArgs a)
{
    extern __shared__ double ur_lds[];
    constexpr int NPIX = kUnringMax / 16;
    const UnringLines &L = a.L;
    const int n = L.n, pad = (n + kUnringTile - 1) / kUnringTile * kUnringTile;
    double *F = ur_lds, *G = ur_lds + (size_t)pad * kUnringLd, *Dj = ur_lds + (size_t)2 * pad * kUnringLd;
    const int s = blockIdx.x / L.groups, l0 = (blockIdx.x - s * L.groups) * kUnringLines;
    const size_t base = (size_t)s * L.plane;
    ur_stage(F, a.src, a.sub, L, base, l0, pad);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, h = lane >> 4;
    const int l = threadIdx.x & 15, xq = threadIdx.x >> 4;
    double best[NPIX], val[NPIX];
#pragma unroll
    for (int i = 0; i < NPIX; i++) { best[i] = __builtin_inf(); val[i] = 0.0; }
    ur_windows<NPIX>(F, n, xq, l, 0.0, best, val);                // s = 0: the line itself
    for (int j = 1; j < kUnringShifts; j++) {
        for (int t = threadIdx.x; t < n; t += kUnringThreads) Dj[t] = a.D[(size_t)j * n + t];
        __syncthreads();                                         // (and every wavefront is through with the windows of shift j - 1)
        for (int m = wave; m < pad / kUnringTile; m += kUnringThreads / 64) {
            ur_v4d acc = {0.0, 0.0, 0.0, 0.0};
            // A[row][k] = d_j[(row - k) mod n]: the cyclic index wraps at n, never at the padded length; the columns k >= n meet rows of
            // zeros in F, the rows >= n are never read back
            int idx = ((kUnringTile * m + c - h) % n + n) % n;
            for (int ks = 0; ks < pad / kUnringK; ks++) {
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Dj[idx], F[(kUnringK * ks + h) * kUnringLd + c], acc, 0, 0, 0);
                idx -= kUnringK;
                if (idx < 0) idx += n;
            }
#pragma unroll
            for (int g = 0; g < 4; g++) G[(kUnringTile * m + h + 4 * g) * kUnringLd + c] = acc[g];
        }
        __syncthreads();
        const double sj = j <= 20 ? (double)j / 40.0 : -(double)(j - 20) / 40.0;
        ur_windows<NPIX>(G, n, xq, l, sj, best, val);
    }
    if (l0 + l < L.n_lines) {
#pragma unroll
        for (int i = 0; i < NPIX; i++) {
            const int x = xq + 16 * i;
            if (x < n) {
                const size_t at = base + (size_t)(l0 + l) * L.ls + (size_t)x * L.es;
                a.dst[at] = a.add ? a.add[at] + val[i] : val[i];
            }
        }
    }
}

}  // namespace amx

using namespace amx;

extern "C" {

int amx_unring_route(int n_a, int n_b, int64_t out[AMX_UNRING_ROUTE_WORDS])
{
    if (!out) return AMX_E_BADARG;
    const UnringRoute rt = unring_route(n_a, n_b);
    out[0] = rt.ok; out[1] = kUnringTile; out[2] = kUnringLines; out[3] = kUnringK; out[4] = rt.pad_a; out[5] = rt.pad_b;
    out[6] = rt.groups_a; out[7] = rt.groups_b; out[8] = (int64_t)rt.lds_dft; out[9] = (int64_t)rt.lds_shift;
    out[10] = (int64_t)rt.table_bytes; out[11] = (int64_t)rt.slice_bytes; out[12] = rt.chunk; out[13] = (int64_t)kUnringScratchCap;
    return rt.ok ? AMX_OK : AMX_E_BADARG;
}

int amx_prep_unring_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, float *d_out, int axis_a, int axis_b, int64_t *slices,
                           int64_t *passed_through, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_unring: not a plan of this ctx");
    if (axis_a < 0 || axis_a > 2 || axis_b < 0 || axis_b > 2 || axis_a == axis_b)
        return amx_bad(ctx, "amx_prep_unring: the axes must be two different spatial axes out of 0, 1, 2");
    if (!d_img || !d_out) return amx_bad(ctx, "amx_prep_unring: null buffer");
    {
        const char *i0 = (const char *)d_img, *o0 = (const char *)d_out;
        const size_t len = (size_t)p->extent * 4;
        if (i0 < o0 + len && o0 < i0 + len) return amx_bad(ctx, "amx_prep_unring: d_out overlaps the image (every pixel of a slice reads the whole slice)");
    }
    int ka = 0, kb = 0, kc = 0;
    for (int k = 0; k < 3; k++) {
        if (p->ax[k] == axis_a) ka = k;
        else if (p->ax[k] == axis_b) kb = k;
        else kc = k;
    }
    const long long na = p->d[ka], nb = p->d[kb], nc = p->d[kc];
    const UnringRoute rt = unring_route((int)(na > INT_MAX ? 0 : na), (int)(nb > INT_MAX ? 0 : nb));
    if (!rt.ok) return amx_bad(ctx, "amx_prep_unring: an in-plane extent is outside the limit (each must be 8 to 256 pixels)");
    const long long n_slices = nc * p->nS;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)hip_stream;
    const long long S = n_slices < rt.chunk ? n_slices : rt.chunk;
    const size_t plane = (size_t)S * na * nb;
    int rc;
    if ((rc = amx_ensure(ctx, ctx->unring_ws, rt.table_bytes + (size_t)S * rt.slice_bytes))) return rc;
    // layout: 512 bytes of head (the counter), the tables, the chunk's flags (8 bytes a slice), the planes
    char *ws = (char *)ctx->unring_ws.p;
    unsigned long long *counter = (unsigned long long *)ws;
    double *Ca = (double *)(ws + 512), *Sa = Ca + na * na, *Cb = Sa + na * na, *Sb = Cb + nb * nb;
    double *Da = Sb + nb * nb, *Db = Da + kUnringShifts * na;
    int *flags = (int *)(Db + kUnringShifts * nb);
    double *W = (double *)(flags + 2 * S), *Pr = W + plane, *Pi = Pr + plane, *Xr = Pi + plane, *Xi = Xr + plane;
    HIPCHK(ctx, hipMemsetAsync(counter, 0, 8, s));
    hipLaunchKernelGGL(k_unring_tables, dim3((unsigned)((na * na + kUnringShifts * na + 255) / 256)), dim3(256), 0, s, Ca, Sa, Da, (int)na);
    hipLaunchKernelGGL(k_unring_tables, dim3((unsigned)((nb * nb + kUnringShifts * nb + 255) / 256)), dim3(256), 0, s, Cb, Sb, Db, (int)nb);
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_unring_dft), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rt.lds_dft));
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_unring_shift), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rt.lds_shift));
    UnringGeo g;
    g.sa = p->s[ka]; g.sb = p->s[kb]; g.sc = p->s[kc]; g.sv = p->sv; g.na = (int)na; g.nb = (int)nb; g.nS = p->nS;
    g.order = (p->sv < g.sa && p->sv < g.sb && p->nS > 1) ? 2 : (g.sa < g.sb ? 1 : 0);
    const UnringLines along_a = {(int)na, (int)nb, rt.groups_a, nb, 1, na * nb}, along_b = {(int)nb, (int)na, rt.groups_b, 1, nb, na * nb};
    for (long long slice0 = 0; slice0 < n_slices; slice0 += S) {
        const int Sc = (int)(n_slices - slice0 < S ? n_slices - slice0 : S);
        const unsigned eb = (unsigned)(((long long)Sc * na * nb + 255) / 256);
        HIPCHK(ctx, hipMemsetAsync(flags, 0, (size_t)Sc * 4, s));
        hipLaunchKernelGGL(k_unring_gather, dim3(eb), dim3(256), 0, s, d_img, W, flags, counter, g, slice0, Sc);
        UnringDftArgs d;
        d = {W, nullptr, Pr, Pi, Cb, Sb, nullptr, 0, 1.0, 0, 1.0, along_b};
        hipLaunchKernelGGL(k_unring_dft, dim3((unsigned)(Sc * rt.groups_b)), dim3(kUnringThreads), rt.lds_dft, s, d);
        d = {Pr, Pi, Xr, Xi, Ca, Sa, Cb, (int)nb, 1.0, 1, 1.0, along_a};
        hipLaunchKernelGGL(k_unring_dft, dim3((unsigned)(Sc * rt.groups_a)), dim3(kUnringThreads), rt.lds_dft, s, d);
        d = {Xr, Xi, Pr, Pi, Ca, Sa, nullptr, 0, -1.0, 0, 1.0, along_a};
        hipLaunchKernelGGL(k_unring_dft, dim3((unsigned)(Sc * rt.groups_a)), dim3(kUnringThreads), rt.lds_dft, s, d);
        d = {Pr, Pi, Xr, nullptr, Cb, Sb, nullptr, 0, -1.0, 2, 1.0 / ((double)na * (double)nb), along_b};
        hipLaunchKernelGGL(k_unring_dft, dim3((unsigned)(Sc * rt.groups_b)), dim3(kUnringThreads), rt.lds_dft, s, d);
        UnringShiftArgs u;
        u = {Xr, nullptr, nullptr, Pr, Da, along_a};              // U along a of Ix
        hipLaunchKernelGGL(k_unring_shift, dim3((unsigned)(Sc * rt.groups_a)), dim3(kUnringThreads), rt.lds_shift, s, u);
        u = {Xr, W, Pr, Pr, Db, along_b};                         // + U along b of Iy = I - Ix
        hipLaunchKernelGGL(k_unring_shift, dim3((unsigned)(Sc * rt.groups_b)), dim3(kUnringThreads), rt.lds_shift, s, u);
        hipLaunchKernelGGL(k_unring_scatter, dim3(eb), dim3(256), 0, s, d_img, Pr, flags, d_out, g, slice0, Sc);
        HIPCHK(ctx, hipGetLastError());
    }
    for (const char *k : {"k_unring_gather", "k_unring_dft", "k_unring_shift", "k_unring_scatter"}) amx_note(ctx, k);
    unsigned long long bad = 0;
    HIPCHK(ctx, hipMemcpyAsync(&bad, counter, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (slices) *slices = n_slices;
    if (passed_through) *passed_through = (int64_t)bad;
    return AMX_OK;
}

}  // extern "C"
