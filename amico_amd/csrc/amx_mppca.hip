// amx_mppca.hip -- the noise level per voxel by Marchenko-Pastur PCA of its local patch (doEstimateNoise = 'MPPCA'; Veraart et
// al. 2016 with the degrees-of-freedom correction of Cordero-Grande et al. 2019; nothing of the reference's).  include/amico_amd.h fixes the
// arithmetic; tests/mppca_np.py restates it.
//   k_mppca<W>   one team per masked voxel: W = 5 the whole workgroup (four wavefronts), W = 3 one wavefront (four patches per workgroup)
//     1. the cube's masked voxels -> the columns' image offsets (LDS), n of them; 2 n < W^3: every output NaN
//     2. G = X X^T (m <= n) or X^T X (m > n), r x r: the patch is staged 32 samples of every row at a time as float32 T[row][33] and
//        multiplied on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, exact products of widened float32, fp64 sums); a wavefront keeps
//        the accumulators of its 16 x 16 tiles of the lower triangle in registers over all chunks, then writes both triangles
//     3. Householder tridiagonalisation of G in place in LDS (unblocked, full symmetric storage: every access runs along a row)
//     4. Sturm-count bisection, one eigenvalue per lane, 56 halvings of the Gershgorin interval: the bracket ends at 2^-55 of it
//     5. lane 0 walks the rule, takes the centre's b0 mean and writes
//   k_mppca_denoise<W>   the same team and the same five stages (one body, mppca_team), then (doDenoise = 'MPPCA')
//     6. the centre voxel's column of the patch's best approximation of rank n_signal: the reflectors stay where G's rows held them, the
//        eigenvectors of the smaller of the signal and the noise set come from the twisted factorisation, one lane each, into G's dead
//        lower triangle; Gram-Schmidt twice; project, transform back on one wavefront, write the centre's samples
// Every threshold scales with the matrix (the pivot guard is 2^-104 of the Gershgorin bound, the bracket a power-of-two fraction of it): the
// outputs of 2^k img are 2^k times those of img bit for bit.  Every loop is a counted loop (toolchain note).
#include "amx_host.hpp"
#include "amx_mppca_route.hpp"

namespace amx {

typedef double mp_v4d __attribute__((ext_vector_type(4)));

struct MppcaArgs {
    const float *img;
    const int *rank;              // [d2][d1][d0]
    const int *b0idx;             // device, n_b0 entries
    double *sigma, *nsignal, *mean, *ratio, *eig;     // [n_vox] each (eig: [n_vox][125]); any may be null
    long long d0, d1, d2, s0, s1, s2, sv;
    int nS, n_b0;
    // k_mppca_denoise only
    float *out;                   // the denoised image, in the image's layout (a copy of img before the launch)
    int *status;                  // [n_vox]; may be null
    double *rows64;               // [n_vox][nS]; may be null
};

template <int TW> __device__ __forceinline__ void team_sync()
{
    if (TW == 1) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    else __syncthreads();
}

__device__ __forceinline__ double mp_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

constexpr int kBisectSteps = 56;

// vector p of the set of eigenvectors, element i: the vectors live in what the tridiagonalisation left dead of G -- the lower triangle with
// the diagonal (d and e are in vd / ve, the reflectors in the strict upper triangle).  Row p offers p + 1 words and row r - 2 - p the other
// r - 1 - p: (r - 1) / 2 such pairs, and the last row, r words, is one vector more -- never fewer than r / 2, the most the complement
// trick asks for.
__device__ __forceinline__ double *mp_slot(double *G, int ldg, int r, int p, int i)
{
    if (p >= (r - 1) / 2) return G + (size_t)(r - 1) * ldg + i;
    return i <= p ? G + (size_t)p * ldg + i : G + (size_t)(r - 2 - p) * ldg + (i - p - 1);
}

// z <- (I - tau2 v v') z for the reflector row k holds (v = G[k][k+1 ..], over the elements k+1 .. r-1); one wavefront, the lane keeps
// elements lane and lane + 64 of z
__device__ __forceinline__ void mp_reflect(const double *G, int ldg, int r, int k, double tau2, int lane, double &z0, double &z1)
{
    const int e0 = lane, e1 = lane + 64;
    const double v0 = e0 > k && e0 < r ? G[k * ldg + e0] : 0.0, v1 = e1 > k && e1 < r ? G[k * ldg + e1] : 0.0;
    const double f = tau2 * mp_wave_sum(v0 * z0 + v1 * z1);
    z0 -= f * v0; z1 -= f * v1;
}

// DEN: the team goes on to the rank-n_signal reconstruction of its centre voxel (k_mppca_denoise); without it every
// `if constexpr (DEN)` below is no code at all and this is k_mppca as it has always been
template <int W, bool DEN>
__device__ __forceinline__ void mppca_team(const MppcaArgs &a, int per_patch_bytes)
{
    constexpr int W3 = W * W * W, H = (W - 1) / 2;
    constexpr int TW = W == 5 ? 4 : 1;                   // wavefronts per patch
    constexpr int T = 64 * TW;                           // threads per patch
    constexpr int PPW = kMppcaThreads / T;               // patches per workgroup
    constexpr int RPMAX = (W3 + 15) / 16 * 16;           // 128 | 32
    constexpr int NTMAX = RPMAX / 16;
    constexpr int TILES = NTMAX * (NTMAX + 1) / 2;       // 36 | 3
    constexpr int MAXT = (TILES + TW - 1) / TW;          // tiles a wavefront owns: 9 | 3
    constexpr int KC = kMppcaChunk, LD = KC + 1;
    constexpr int CW = RPMAX < 64 ? RPMAX : 64, RPW = 64 / CW;   // the rank-2 update: columns per wavefront pass, rows per pass
    extern __shared__ double mp_lds[];

    const int team = threadIdx.x / T, t = threadIdx.x % T, lane = threadIdx.x & 63, wv = t >> 6;
    const long long vox = (long long)blockIdx.x * PPW + team;
    if (vox >= a.d0 * a.d1 * a.d2) return;               // (uniform over the team; teams of one wavefront never meet a workgroup barrier)
    const int row_out = a.rank[vox];
    if (row_out < 0) return;

    const int m = a.nS;
    const int rmax = m < W3 ? m : W3, rp_max = (rmax + 15) / 16 * 16, ldg = rmax | 1;
    double *G = reinterpret_cast<double *>(reinterpret_cast<char *>(mp_lds) + (size_t)team * per_patch_bytes);
    double *vd = G + (size_t)rmax * ldg, *ve = vd + rp_max, *vv = ve + rp_max, *vw = vv + rp_max, *lam = vw + rp_max, *part = lam + rp_max;
    double *tau = part + 2 * rp_max;                     // DEN: tau2 of every reflector
    long long *off = reinterpret_cast<long long *>(part + (DEN ? 3 : 2) * rp_max);
    float *stage = reinterpret_cast<float *>(off + W3);
    int *state = reinterpret_cast<int *>(stage + (size_t)rp_max * LD);     // [0] n, [1] a sample is not finite
    int *present = reinterpret_cast<int *>(stage);

    // ---- 1. the cube and its masked voxels, in memory-axis order
    const long long c0 = vox % a.d0, c1 = (vox / a.d0) % a.d1, c2 = vox / (a.d0 * a.d1);
    const long long lo0 = c0 - H < 0 ? 0 : (c0 - H > a.d0 - W ? a.d0 - W : c0 - H);
    const long long lo1 = c1 - H < 0 ? 0 : (c1 - H > a.d1 - W ? a.d1 - W : c1 - H);
    const long long lo2 = c2 - H < 0 ? 0 : (c2 - H > a.d2 - W ? a.d2 - W : c2 - H);
    long long my_off = 0;
    int my_in = 0;
    for (int u = t; u < W3; u += T) {                    // (one trip: W3 <= 2 T; W = 3 has 27 <= 64, W = 5 has 125 <= 256)
        const long long i0 = lo0 + u % W, i1 = lo1 + (u / W) % W, i2 = lo2 + u / (W * W);
        my_in = a.rank[(i2 * a.d1 + i1) * a.d0 + i0] >= 0;
        my_off = i0 * a.s0 + i1 * a.s1 + i2 * a.s2;
        present[u] = my_in;
    }
    if (t == 0) state[1] = 0;
    team_sync<TW>();
    if (t < W3) {
        int pos = 0;
        for (int u = 0; u < t; u++) pos += present[u];
        if (my_in) off[pos] = my_off;
        if (t == W3 - 1) state[0] = pos + my_in;
        if (DEN && t == (int)((c0 - lo0) + (c1 - lo1) * W + (c2 - lo2) * W * W)) state[4] = pos;     // the centre's column
    }
    team_sync<TW>();
    const int n = state[0];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    bool eligible = 2 * n >= W3;
    const int r = m < n ? m : n, q = m < n ? n : m;
    const bool side_vol = m <= n;                        // rows of the staged tile are volumes, its samples run over the columns
    const int ntr = (r + 15) / 16;

    if (eligible) {
        // ---- 2. the Gram matrix
        mp_v4d acc[MAXT];
#pragma unroll
        for (int u = 0; u < MAXT; u++) acc[u] = (mp_v4d){0.0, 0.0, 0.0, 0.0};
        const bool fast_row = side_vol == (a.sv == 1);   // consecutive threads take consecutive rows when that is the contiguous direction
        const int rp = ntr * 16;
        bool bad = false;
        for (int k0 = 0; k0 < q; k0 += KC) {
            team_sync<TW>();                             // the previous chunk's products have read the tile (and `present` is done with)
            for (int e = t; e < rp * KC; e += T) {
                const int row = fast_row ? e % rp : e / KC, kk = fast_row ? e / rp : e % KC;
                float x = 0.0f;
                if (row < r && k0 + kk < q) {
                    const int vol = side_vol ? row : k0 + kk, col = side_vol ? k0 + kk : row;
                    x = a.img[off[col] + (long long)vol * a.sv];
                    bad = bad || !(fabsf(x) < INFINITY);
                }
                stage[row * LD + kk] = x;
            }
            team_sync<TW>();
#pragma unroll
            for (int u = 0; u < MAXT; u++) {
                const int id = wv + u * TW;
                int ti = 0, tj = id;
                for (int g = 0; g < NTMAX; g++) if (tj > ti) { tj -= ti + 1; ti++; }     // tile id -> (ti >= tj) of the lower triangle
                if (id < TILES && ti < ntr) {
                    const float *pa = stage + (16 * ti + (lane & 15)) * LD + (lane >> 4);
                    const float *pb = stage + (16 * tj + (lane & 15)) * LD + (lane >> 4);
#pragma unroll
                    for (int ks = 0; ks < KC / 4; ks++)
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)pa[4 * ks], (double)pb[4 * ks], acc[u], 0, 0, 0);
                }
            }
        }
        if (bad) state[1] = 1;
#pragma unroll
        for (int u = 0; u < MAXT; u++) {
            const int id = wv + u * TW;
            int ti = 0, tj = id;
            for (int g = 0; g < NTMAX; g++) if (tj > ti) { tj -= ti + 1; ti++; }
            if (id < TILES && ti < ntr) {
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int i = 16 * ti + (lane >> 4) + 4 * g, j = 16 * tj + (lane & 15);
                    if (i < r && j < r) {
                        G[i * ldg + j] = acc[u][g];
                        if (ti != tj) G[j * ldg + i] = acc[u][g];
                    }
                }
            }
        }
        team_sync<TW>();
        eligible = state[1] == 0;
    }

    if (eligible) {
        // ---- 3. Householder tridiagonalisation: d = vd, e = ve
        for (int k = 0; k + 2 < r; k++) {
            const int b = k + 1, nn = r - b;
            const double xj = t < nn ? G[k * ldg + b + t] : 0.0;
            const double ss = mp_wave_sum(xj * xj);
            if (lane == 0 && wv < 2) part[wv] = ss;
            team_sync<TW>();
            const double sigma2 = TW > 1 ? part[0] + part[1] : part[0];
            const double x0 = G[k * ldg + b];
            const double norm = sqrt(sigma2);
            const double alpha = x0 >= 0.0 ? -norm : norm;
            if (t == 0) { vd[k] = G[k * ldg + k]; ve[k] = sigma2 > 0.0 ? alpha : 0.0; }
            if (DEN && t == 0) tau[k] = sigma2 > 0.0 ? 1.0 / (sigma2 - alpha * x0) : 0.0;
            if (!(sigma2 > 0.0)) { team_sync<TW>(); continue; }      // nothing below the diagonal: no reflector (uniform over the team)
            const double tau2 = 1.0 / (sigma2 - alpha * x0);         // 2 / v'v, v = x - alpha e1: alpha x0 <= 0, nothing cancels
            if (t < nn) vv[t] = t == 0 ? x0 - alpha : xj;
            team_sync<TW>();
            {   // p = tau2 A v: thread (h, j) sums its half of the rows of column j
                const int j = t % rp_max, h = t / rp_max;            // (T / rp_max >= 2 halves: 256 / 128, 64 / 32 or more)
                if (h < 2) {
                    const int half = (nn + 1) / 2, i0 = h * half, i1 = h == 0 ? half : nn;
                    double s = 0.0;
                    if (j < nn) for (int i = i0; i < i1; i++) s += G[(b + i) * ldg + b + j] * vv[i];
                    part[h * rp_max + j] = s;
                }
            }
            team_sync<TW>();
            const double pj = t < nn ? tau2 * (part[t] + part[rp_max + t]) : 0.0;
            const double vj = t < nn ? vv[t] : 0.0;
            const double vp = mp_wave_sum(vj * pj);
            team_sync<TW>();                                         // everyone has read part[] before it is written again
            if (lane == 0 && wv < 2) part[wv] = vp;
            team_sync<TW>();
            const double Kc = 0.5 * tau2 * (TW > 1 ? part[0] + part[1] : part[0]);
            if (t < nn) vw[t] = pj - Kc * vj;
            if (DEN && t == 0) G[k * ldg + b] = x0 - alpha;         // row k keeps the reflector (everyone has read x0 by now)
            team_sync<TW>();
            {   // A -= v w' + w v', both triangles; products rounded on their own so that (i, j) and (j, i) get the same bits
#pragma clang fp contract(off)
                const int cc = (nn + CW - 1) / CW, tasks = ((nn + RPW - 1) / RPW) * cc;
                for (int task = wv; task < tasks; task += TW) {
                    const int i = (task / cc) * RPW + lane / CW, j = (task % cc) * CW + lane % CW;
                    if (i < nn && j < nn) {
                        const double t1 = vv[i] * vw[j], t2 = vw[i] * vv[j];
                        G[(b + i) * ldg + b + j] -= t1 + t2;
                    }
                }
            }
            team_sync<TW>();
        }
        if (t == 0) {
            if (r >= 2) { vd[r - 2] = G[(r - 2) * ldg + r - 2]; ve[r - 2] = G[(r - 1) * ldg + r - 2]; }
            vd[r - 1] = G[(r - 1) * ldg + r - 1];
        }
        team_sync<TW>();

        // ---- 4. bisection: lane t finds eigenvalue t (ascending)
        if (t < r) {
            double glo = 0.0, ghi = 0.0;
            for (int i = 0; i < r; i++) {
                const double rad = (i > 0 ? fabs(ve[i - 1]) : 0.0) + (i + 1 < r ? fabs(ve[i]) : 0.0);
                const double l_ = vd[i] - rad, h_ = vd[i] + rad;
                glo = i == 0 ? l_ : fmin(glo, l_); ghi = i == 0 ? h_ : fmax(ghi, h_);
            }
            const double bnd = fmax(fabs(glo), fabs(ghi));
            const double pivmin = bnd * 0x1p-104;
            double lo = glo - bnd * 0x1p-40, hi = ghi + bnd * 0x1p-40;
            for (int it = 0; it < kBisectSteps; it++) {
                const double mid = 0.5 * (lo + hi);
                int cnt = 0;
                double qq = vd[0] - mid;
                if (fabs(qq) < pivmin) qq = -pivmin;
                cnt += qq < 0.0;
                for (int i = 1; i < r; i++) {
                    const double e_ = ve[i - 1];
                    qq = vd[i] - mid - e_ * e_ / qq;
                    if (fabs(qq) < pivmin) qq = -pivmin;
                    cnt += qq < 0.0;
                }
                if (cnt > t) hi = mid; else lo = mid;
            }
            lam[t] = 0.5 * (lo + hi);
        }
        team_sync<TW>();
    }

    // ---- 5. the rule and the centre's b0 mean (lane 0), then the outputs
    if (t == 0) {
        double sigma = nan, nsig = nan, mean = nan;
        if (eligible) {
            const double l0 = fmax(lam[0], 0.0) / (double)q;
            double S = 0.0, var = 0.0;
            int cut = 0;
            for (int p = 0; p < r; p++) {
                const double lp = fmax(lam[p], 0.0) / (double)q;
                S += lp;
                const double gam = (double)(p + 1) / (double)(q - (r - p - 1));
                const double s1 = S / (double)(p + 1);
                const double s2 = (lp - l0) / (4.0 * sqrt(gam));
                if (s2 < s1) { var = s1; cut = p + 1; }
            }
            if (cut > 0) { sigma = sqrt(var); nsig = (double)(r - cut); }
            else eligible = false;
        }
        if (eligible && a.n_b0 > 0) {
#pragma clang fp contract(off)
            const float *src = a.img + c0 * a.s0 + c1 * a.s1 + c2 * a.s2;
            double sum = 0.0;
            for (int i = 0; i < a.n_b0; i++) {
                const double x = (double)src[(long long)a.b0idx[i] * a.sv];
                sum = i == 0 ? x : sum + x;
            }
            const double mu = sum / (double)a.n_b0;
            if (mu > 0.0) mean = mu;
        }
        if (a.sigma) a.sigma[row_out] = sigma;
        if (a.nsignal) a.nsignal[row_out] = nsig;
        if (a.mean) a.mean[row_out] = mean;
        if (a.ratio) a.ratio[row_out] = mean / sigma;
        state[2] = eligible;                             // (a voxel the rule finds no p for is NaN in its eigenvalues as well)
        if (DEN) state[3] = eligible ? r - (int)nsig : 0;
    }
    team_sync<TW>();
    eligible = state[2] != 0;
    if (a.eig) for (int u = t; u < kMppcaMaxSide; u += T) a.eig[(size_t)row_out * kMppcaMaxSide + u] = eligible && u < r ? lam[u] : nan;

    if constexpr (DEN) {
        // ---- 6. the centre's column of the best rank-s approximation of X, s = r - cut (include/amico_amd.h, "(f0+++)")
        if (t == 0 && a.status) a.status[row_out] = eligible ? 0 : 1;
        if (!eligible) {                                 // passed through: d_out holds the copy of the image
            if (a.rows64) for (int u = t; u < m; u += T) a.rows64[(size_t)row_out * m + u] = nan;
            return;
        }
        const long long coff = c0 * a.s0 + c1 * a.s1 + c2 * a.s2;
        const int cut = state[3], s = r - cut, ccol = state[4];
        const bool use_sig = s <= cut;                   // the smaller set: the signal vectors, or the noise vectors and the complement
        const int ks = use_sig ? s : cut, first = use_sig ? cut : 0;
        double *bp = vv, *zz = vw, *cf = part;           // (free since the tridiagonalisation)
        const int e0 = lane, e1 = lane + 64;             // the two elements of an r-vector a lane of wavefront 0 keeps (r <= 125)
        if (ks > 0) {
            if (wv == 0) {                               // b' = Q^T b, b = x_c | e_c: the reflectors in order
                double z0 = 0.0, z1 = 0.0;
                if (side_vol) {
                    if (e0 < r) z0 = (double)a.img[coff + (long long)e0 * a.sv];
                    if (e1 < r) z1 = (double)a.img[coff + (long long)e1 * a.sv];
                } else {
                    z0 = e0 == ccol ? 1.0 : 0.0; z1 = e1 == ccol ? 1.0 : 0.0;
                }
                for (int k = 0; k + 2 < r; k++) mp_reflect(G, ldg, r, k, tau[k], lane, z0, z1);
                if (e0 < r) bp[e0] = z0;
                if (e1 < r) bp[e1] = z1;
            }
            if (t < ks) {
                // the tridiagonal's eigenvector of lam[first + t] by the twisted factorisation, into slot t; the pivots are kept
                // 2^-104 of the Gershgorin bound away from zero as the Sturm count's are
                double glo = 0.0, ghi = 0.0;
                for (int i = 0; i < r; i++) {
                    const double rad = (i > 0 ? fabs(ve[i - 1]) : 0.0) + (i + 1 < r ? fabs(ve[i]) : 0.0);
                    const double l_ = vd[i] - rad, h_ = vd[i] + rad;
                    glo = i == 0 ? l_ : fmin(glo, l_); ghi = i == 0 ? h_ : fmax(ghi, h_);
                }
                const double pivmin = fmax(fabs(glo), fabs(ghi)) * 0x1p-104;
                const double lm = lam[first + t];
                double dp = vd[0] - lm;                  // forward pivots
                if (fabs(dp) < pivmin) dp = -pivmin;
                *mp_slot(G, ldg, r, t, 0) = dp;
                for (int i = 1; i < r; i++) {
                    const double e_ = ve[i - 1];
                    dp = vd[i] - lm - e_ * e_ / dp;
                    if (fabs(dp) < pivmin) dp = -pivmin;
                    *mp_slot(G, ldg, r, t, i) = dp;
                }
                double dm = vd[r - 1] - lm;              // backward pivots: gamma_i = dp_i + dm_i - (d_i - lam), the twist at its smallest
                if (fabs(dm) < pivmin) dm = -pivmin;
                int tw = r - 1;
                double gmin = fabs(dp + dm - (vd[r - 1] - lm));
                for (int ii = 1; ii < r; ii++) {
                    const int i = r - 1 - ii;
                    const double e_ = ve[i];
                    dm = vd[i] - lm - e_ * e_ / dm;
                    if (fabs(dm) < pivmin) dm = -pivmin;
                    const double g = fabs(*mp_slot(G, ldg, r, t, i) + dm - (vd[i] - lm));
                    if (g < gmin) { gmin = g; tw = i; }
                }
                dm = vd[r - 1] - lm;                     // once more, kept above the twist
                if (fabs(dm) < pivmin) dm = -pivmin;
                if (r - 1 > tw) *mp_slot(G, ldg, r, t, r - 1) = dm;
                for (int ii = 1; ii < r; ii++) {
                    const int i = r - 1 - ii;
                    const double e_ = ve[i];
                    dm = vd[i] - lm - e_ * e_ / dm;
                    if (fabs(dm) < pivmin) dm = -pivmin;
                    if (i > tw) *mp_slot(G, ldg, r, t, i) = dm;
                }
                double z = 1.0;                          // z_tw = 1; below it by the forward pivots, above it by the backward ones
                for (int ii = 0; ii < r; ii++) {
                    const int i = tw - 1 - ii;
                    if (i >= 0) { double *p_ = mp_slot(G, ldg, r, t, i); z = -ve[i] * z / *p_; *p_ = z; }
                }
                z = 1.0;
                for (int i = 1; i < r; i++)
                    if (i > tw) { double *p_ = mp_slot(G, ldg, r, t, i); z = -ve[i - 1] * z / *p_; *p_ = z; }
                *mp_slot(G, ldg, r, t, tw) = 1.0;
            }
            team_sync<TW>();
            // orthonormal by Gram-Schmidt, every vector twice against those before it: lane i takes the product with u_i, then lane e
            // element e of the sum
            for (int j = 0; j < ks; j++) {
                for (int pass = 0; pass < 2 && j > 0; pass++) {
                    if (t < j) {
                        double d_ = 0.0;
                        for (int i = 0; i < r; i++) d_ += *mp_slot(G, ldg, r, t, i) * *mp_slot(G, ldg, r, j, i);
                        cf[t] = d_;
                    }
                    team_sync<TW>();
                    if (t < r) {
                        double acc = 0.0;
                        for (int i = 0; i < j; i++) acc += cf[i] * *mp_slot(G, ldg, r, i, t);
                        *mp_slot(G, ldg, r, j, t) -= acc;
                    }
                    team_sync<TW>();
                }
                if (wv == 0) {
                    double *p0 = mp_slot(G, ldg, r, j, e0 < r ? e0 : 0), *p1 = mp_slot(G, ldg, r, j, e1 < r ? e1 : 0);
                    const double u0 = e0 < r ? *p0 : 0.0, u1 = e1 < r ? *p1 : 0.0;
                    const double ss = mp_wave_sum(u0 * u0 + u1 * u1);
                    const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
                    if (e0 < r) *p0 = u0 * inv;
                    if (e1 < r) *p1 = u1 * inv;
                }
                team_sync<TW>();
            }
            // z' = P b' (the signal set) | b' - P b' (the noise set)
            if (t < ks) {
                double d_ = 0.0;
                for (int i = 0; i < r; i++) d_ += *mp_slot(G, ldg, r, t, i) * bp[i];
                cf[t] = d_;
            }
            team_sync<TW>();
            if (wv == 0) {                               // z = Q z': the reflectors in reverse order
                double z0 = 0.0, z1 = 0.0;
                for (int i = 0; i < ks; i++) {
                    if (e0 < r) z0 += cf[i] * *mp_slot(G, ldg, r, i, e0);
                    if (e1 < r) z1 += cf[i] * *mp_slot(G, ldg, r, i, e1);
                }
                if (!use_sig) { z0 = e0 < r ? bp[e0] - z0 : 0.0; z1 = e1 < r ? bp[e1] - z1 : 0.0; }
                for (int kk = 0; kk + 2 < r; kk++) mp_reflect(G, ldg, r, r - 3 - kk, tau[r - 3 - kk], lane, z0, z1);
                if (e0 < r) zz[e0] = z0;
                if (e1 < r) zz[e1] = z1;
            }
            team_sync<TW>();
        }
        // volumes side: x^ = z; patch side: x^ = X z, the patch read once more.  s = 0: the rank-0 reconstruction, zeros
        for (int vol = t; vol < m; vol += T) {
            double x = 0.0;
            if (ks > 0) {
                if (side_vol) x = zz[vol];
                else for (int col = 0; col < n; col++) x += (double)a.img[off[col] + (long long)vol * a.sv] * zz[col];
            }
            a.out[coff + (long long)vol * a.sv] = (float)x;
            if (a.rows64) a.rows64[(size_t)row_out * m + vol] = x;
        }
    }
}

template <int W>
__global__ __launch_bounds__(kMppcaThreads) void k_mppca(MppcaArgs a, int per_patch_bytes)
{
    mppca_team<W, false>(a, per_patch_bytes);
}

template <int W>
__global__ __launch_bounds__(kMppcaThreads) void k_mppca_denoise(MppcaArgs a, int per_patch_bytes)
{
    mppca_team<W, true>(a, per_patch_bytes);
}

}  // namespace amx

using namespace amx;

extern "C" {

int amx_mppca_route(int nS, int patch, int n_cols, const int64_t dims[3], int64_t out[AMX_MPPCA_ROUTE_WORDS])
{
    if (!out || !dims) return AMX_E_BADARG;
    const MppcaRoute rt = mppca_route(nS, patch, n_cols, dims[0], dims[1], dims[2]);
    out[0] = rt.ok; out[1] = rt.r; out[2] = rt.q; out[3] = rt.side; out[4] = rt.gram; out[5] = rt.chunk; out[6] = rt.waves;
    out[7] = rt.patches; out[8] = (int64_t)rt.lds; out[9] = rt.eligible;
    return rt.ok ? AMX_OK : AMX_E_BADARG;
}

int amx_prep_noise_mppca_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, int patch, double *d_sigma, double *d_nsignal,
                                double *d_mean, double *d_ratio, double *d_eig, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_noise_mppca: not a plan of this ctx");
    if (patch != 3 && patch != 5) return amx_bad(ctx, "amx_prep_noise_mppca: the patch edge must be 3 or 5");
    if (p->nS > kMppcaMaxVolumes) return amx_bad(ctx, "amx_prep_noise_mppca: scheme too long (at most 512 volumes)");
    if (p->d[0] < patch || p->d[1] < patch || p->d[2] < patch) return amx_bad(ctx, "amx_prep_noise_mppca: an axis of the volume is shorter than the patch");
    if (!d_sigma && !d_nsignal && !d_mean && !d_ratio && !d_eig)
        return amx_bad(ctx, "amx_prep_noise_mppca: no output buffer (give at least one of sigma, n_signal, mean, ratio, eig)");
    if (p->n_vox == 0) return amx_bad(ctx, "amx_prep_noise_mppca: the plan has no masked voxel");
    if (!d_img) return amx_bad(ctx, "amx_prep_noise_mppca: null buffer");
    {   // outputs may not overlap: each is written by another lane, in no order
        const char *b[5] = {(const char *)d_sigma, (const char *)d_nsignal, (const char *)d_mean, (const char *)d_ratio, (const char *)d_eig};
        const size_t len[5] = {(size_t)p->n_vox * 8, (size_t)p->n_vox * 8, (size_t)p->n_vox * 8, (size_t)p->n_vox * 8, (size_t)p->n_vox * 8 * kMppcaMaxSide};
        for (int i = 0; i < 5; i++)
            for (int j = i + 1; j < 5; j++)
                if (b[i] && b[j] && b[i] < b[j] + len[j] && b[j] < b[i] + len[i]) return amx_bad(ctx, "amx_prep_noise_mppca: output buffers overlap");
    }
    const MppcaRoute rt = mppca_route(p->nS, patch, patch * patch * patch, p->d[0], p->d[1], p->d[2]);
    if (!rt.ok) return amx_bad(ctx, "amx_prep_noise_mppca: no route for this shape");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    MppcaArgs a;
    memset(&a, 0, sizeof a);
    a.img = d_img; a.rank = p->rank; a.b0idx = p->b0idx;
    a.sigma = d_sigma; a.nsignal = d_nsignal; a.mean = d_mean; a.ratio = d_ratio; a.eig = d_eig;
    a.d0 = p->d[0]; a.d1 = p->d[1]; a.d2 = p->d[2]; a.s0 = p->s[0]; a.s1 = p->s[1]; a.s2 = p->s[2]; a.sv = p->sv;
    a.nS = p->nS; a.n_b0 = p->n_b0;
    const long long blocks = (p->n_total + rt.patches - 1) / rt.patches;
    hipStream_t s = (hipStream_t)hip_stream;
    if (patch == 5) {
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mppca<5>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rt.lds));
        hipLaunchKernelGGL((k_mppca<5>), dim3((unsigned)blocks), dim3(kMppcaThreads), rt.lds, s, a, (int)rt.per_patch);
    } else {
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mppca<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rt.lds));
        hipLaunchKernelGGL((k_mppca<3>), dim3((unsigned)blocks), dim3(kMppcaThreads), rt.lds, s, a, (int)rt.per_patch);
    }
    HIPCHK(ctx, hipGetLastError());
    amx_note(ctx, patch == 5 ? "k_mppca<5>" : "k_mppca<3>");
    return AMX_OK;
}

int amx_mppca_denoise_route(int nS, int patch, int n_cols, const int64_t dims[3], int64_t out[AMX_MPPCA_DENOISE_ROUTE_WORDS])
{
    if (!out || !dims) return AMX_E_BADARG;
    const MppcaDenoiseRoute rt = mppca_denoise_route(nS, patch, n_cols, dims[0], dims[1], dims[2]);
    out[0] = rt.ok; out[1] = rt.r; out[2] = rt.q; out[3] = rt.side; out[4] = rt.waves; out[5] = rt.patches; out[6] = (int64_t)rt.per_patch;
    out[7] = (int64_t)rt.lds; out[8] = rt.capacity; out[9] = rt.cap; out[10] = rt.eligible;
    return rt.ok ? AMX_OK : AMX_E_BADARG;
}

int amx_prep_noise_mppca_denoise_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, int patch, float *d_out, double *d_sigma,
                                        double *d_nsignal, double *d_mean, double *d_ratio, int *d_status, double *d_rows64, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!p || p->ctx != ctx) return amx_bad(ctx, "amx_prep_noise_mppca_denoise: not a plan of this ctx");
    if (patch != 3 && patch != 5) return amx_bad(ctx, "amx_prep_noise_mppca_denoise: the patch edge must be 3 or 5");
    if (p->nS > kMppcaMaxVolumes) return amx_bad(ctx, "amx_prep_noise_mppca_denoise: scheme too long (at most 512 volumes)");
    if (p->d[0] < patch || p->d[1] < patch || p->d[2] < patch)
        return amx_bad(ctx, "amx_prep_noise_mppca_denoise: an axis of the volume is shorter than the patch");
    if (p->n_vox == 0) return amx_bad(ctx, "amx_prep_noise_mppca_denoise: the plan has no masked voxel");
    if (!d_img || !d_out) return amx_bad(ctx, "amx_prep_noise_mppca_denoise: null buffer (the image and d_out are required)");
    {   // the patches overlap, so the image is read while d_out is written; and every output is written by another lane, in no order
        const char *all[8] = {(const char *)d_img, (const char *)d_out, (const char *)d_sigma, (const char *)d_nsignal, (const char *)d_mean,
                              (const char *)d_ratio, (const char *)d_status, (const char *)d_rows64};
        const size_t nv = (size_t)p->n_vox;
        const size_t len[8] = {(size_t)p->extent * 4, (size_t)p->extent * 4, nv * 8, nv * 8, nv * 8, nv * 8, nv * 4, nv * 8 * (size_t)p->nS};
        for (int i = 0; i < 8; i++)
            for (int j = i + 1; j < 8; j++)
                if (all[i] && all[j] && all[i] < all[j] + len[j] && all[j] < all[i] + len[i])
                    return amx_bad(ctx, i == 0 ? "amx_prep_noise_mppca_denoise: an output buffer overlaps the image (d_out may not be the image: "
                                                 "the patches overlap)"
                                               : "amx_prep_noise_mppca_denoise: output buffers overlap");
    }
    const MppcaDenoiseRoute rt = mppca_denoise_route(p->nS, patch, patch * patch * patch, p->d[0], p->d[1], p->d[2]);
    if (!rt.ok) return amx_bad(ctx, "amx_prep_noise_mppca_denoise: no route for this shape");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)hip_stream;
    // every sample the kernel does not denoise is the image's: outside the mask, not eligible
    HIPCHK(ctx, hipMemcpyAsync(d_out, d_img, (size_t)p->extent * 4, hipMemcpyDeviceToDevice, s));
    MppcaArgs a;
    memset(&a, 0, sizeof a);
    a.img = d_img; a.rank = p->rank; a.b0idx = p->b0idx;
    a.sigma = d_sigma; a.nsignal = d_nsignal; a.mean = d_mean; a.ratio = d_ratio;
    a.out = d_out; a.status = d_status; a.rows64 = d_rows64;
    a.d0 = p->d[0]; a.d1 = p->d[1]; a.d2 = p->d[2]; a.s0 = p->s[0]; a.s1 = p->s[1]; a.s2 = p->s[2]; a.sv = p->sv;
    a.nS = p->nS; a.n_b0 = p->n_b0;
    const long long blocks = (p->n_total + rt.patches - 1) / rt.patches;
    if (patch == 5) {
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mppca_denoise<5>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rt.lds));
        hipLaunchKernelGGL((k_mppca_denoise<5>), dim3((unsigned)blocks), dim3(kMppcaThreads), rt.lds, s, a, (int)rt.per_patch);
    } else {
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mppca_denoise<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rt.lds));
        hipLaunchKernelGGL((k_mppca_denoise<3>), dim3((unsigned)blocks), dim3(kMppcaThreads), rt.lds, s, a, (int)rt.per_patch);
    }
    HIPCHK(ctx, hipGetLastError());
    amx_note(ctx, patch == 5 ? "k_mppca_denoise<5>" : "k_mppca_denoise<3>");
    return AMX_OK;
}

}  // extern "C"
