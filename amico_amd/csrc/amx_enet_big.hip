// amx_enet_big.hip -- FreeWater, SANDI and CylinderZeppelinBall on dictionaries of 65 .. 256 atoms: whatever model.set() produces.
//
// The wavefront-per-voxel kernels of these models hold 64 atoms (a lane per atom, a 64-bit mask of the passive set) and the optimum of a finer grid
// is not sparse (CylinderZeppelinBall, lambda2 = 4, 130 atoms: 91 passive on average), so this is a dense route: one WORKGROUP of 256 threads per
// voxel, thread = atom, the single lasso of the model
//     min_{x >= 0} 1/2 ||y - A_d x||^2 + lambda1 sum(x) + lambda2/2 ||x||^2
// in Gram space by amx_bpp.hpp's loop (block principal pivoting on a packed Cholesky factor: shared with k_batched_big).  H_d = G_d + lambda2 I:
// G_d = A_d'A_d of every orientation lies in HBM, f64 [ndirs][n][ldG], built once per dictionary and only when it has more than 64 atoms
// (k_big_gram; the small dictionaries pay nothing), lambda2 goes onto the diagonal as H_PP is gathered.  c = A_d'y is formed INSIDE the solver
// workgroup from the dictionary's own tile (float32; float64 for SANDI) where it lies: the check on the true problem sweeps that tile anyway, the
// voxels of one orientation are neighbours in the walk, so the tile and H_d are read from L2, and no table of c crosses HBM.  Signals are read in
// place, float64 or float32.
// The first passive set: every atom when lambda1 = 0 and lambda2 >= 1e-2 (CylinderZeppelinBall's default 4: the optimum holds two thirds of the
// atoms and more, block pivoting from the full set removes the rest in two or three factorisations), else the 32 atoms that fit the signal best on
// their own (FreeWater and SANDI at their default ridges 1e-3 / 5e-3 end with a fifth to a third of the atoms passive, and with lambda2 ~ 0 the
// full H is singular: a factorisation of the full set would only feed the rank guard).  1e-2 is the rule k_czb's dense start has always used.
// The voxels are taken in bucket order, perm[0 .. count) with count = the plan's bucketed total ON THE DEVICE (dir_start[ndirs]): a voxel whose
// direction is out of bounds is in no bucket, and nothing behind the count is read (the finding on k_noddi_lasso_big).
// The maps are the model's own arithmetic (models.pyx:1240-1256 / 1570-1612 / 617-640) on block sums of a fixed tree; the error maps come from the
// true residual y - A x the check has formed (SANDI: of the rescaled x against the normalised A, the reference's quirk).
#include "amx_launch.hpp"
#include "amx_bpp.hpp"
using namespace amx;

namespace {

struct EnetBigArgs {
    FitCommon c;
    const double *gram;           // [ndirs][n][ldG]
    int ldG, ndirs;
    const int *count;             // bucketed voxels (device: dir_start[ndirs]), or null: the n_vox voxels in order (SANDI)
    int n_vox;
    int lcap;                     // largest passive set whose packed factor lies in LDS
    double *Lg;                   // global factor blocks [gridDim.x][n (n + 1) / 2], or null (n <= lcap)
    int full_start;
    double *est, *rmse, *nrmse;
    int n_maps;
    int n_a, n_b, n_iso, is_mouse;   // FreeWater: n_a = n_perp; SANDI: n_a = n_rs, n_b = n_in; CylinderZeppelinBall: n_a = n_rs, n_b = n_perp
    double *ycorr, *xiso;            // FreeWater
    const double *norms, *Rs, *d_in, *d_isos;
};

constexpr int kEbThreads = bpp::kThreads;

// G_d = A_d'A_d, one workgroup per (orientation, row): the row's atom is read by every thread, the other atom across the threads
template <typename AT>
__global__ void __launch_bounds__(256) k_big_gram(const AT *__restrict__ tiles, int m, int n, int ldA, int tile_stride, int ldG, double *__restrict__ G)
{
    const int d = blockIdx.x / n, j = blockIdx.x % n, k = threadIdx.x;
    if (k >= ldG) return;
    const AT *At = tiles + (size_t)d * tile_stride;
    double acc = 0.0;
    if (k < n)
        for (int i = 0; i < m; i++) acc += (double)At[(size_t)i * ldA + j] * (double)At[(size_t)i * ldA + k];
    G[((size_t)d * n + j) * ldG + k] = acc;
}

// MODEL: amx_lut::model (2 FreeWater, 3 SANDI, 4 CylinderZeppelinBall)
template <typename AT, int MODEL>
__global__ void __launch_bounds__(kEbThreads) k_enet_big(const EnetBigArgs b)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_eb[];
    const int m = b.c.nS, ldA = b.c.ldA, n = b.c.n_atoms;
    const bpp::Work w = bpp::carve(smem_eb, m, n);
    double *Lg = b.Lg ? b.Lg + (size_t)blockIdx.x * ((size_t)n * (n + 1) / 2) : w.Ll;
    const int tid = threadIdx.x, nt = kEbThreads;
    const AT *tiles = reinterpret_cast<const AT *>(b.c.tiles);
    int cnt = b.count ? *b.count : b.n_vox;
    if (cnt > b.n_vox) cnt = b.n_vox;
    const double nan = __builtin_nan("");

    for (int it = blockIdx.x; it < cnt; it += gridDim.x) {
        const int vox = b.c.perm ? b.c.perm[it] : it;
        const int dic = MODEL == 3 ? 0 : b.c.lutidx[vox];
        if (vox < 0 || vox >= b.n_vox || dic < 0 || dic >= b.ndirs) continue;      // (uniform over the workgroup; the plan never hands one out)
        const AT *At = tiles + (size_t)dic * b.c.tile_stride;
        const double *G = b.gram + (size_t)dic * n * b.ldG;
        __syncthreads();
        if (tid < 16) w.shi[tid] = 0;
        __syncthreads();
        double yy = 0.0;
        for (int i = tid; i < m; i += nt) {
            const double yi = b.c.y32 ? (double)b.c.y32[(size_t)vox * m + i] : b.c.y[(size_t)vox * m + i];
            if (!(fabs(yi) <= 1.79769313486231570e308)) w.shi[4] = 1;
            w.yv[i] = yi; w.rv[i] = yi;
            yy += yi * yi;
        }
        const double ysq = bpp::block_sum(yy, w.part, tid);
        if (w.shi[4]) {                                           // a non-finite sample: NaN maps, this voxel's alone
            for (int k = tid; k < b.n_maps; k += nt) b.est[(size_t)vox * b.n_maps + k] = nan;
            if (tid == 0 && b.rmse) b.rmse[vox] = nan;
            if (tid == 0 && b.nrmse) b.nrmse[vox] = nan;
            if (MODEL == 2 && b.ycorr)
                for (int i = tid; i < m; i += nt) b.ycorr[(size_t)vox * m + i] = nan;
            if (MODEL == 2 && b.xiso)
                for (int k = tid; k < b.n_iso; k += nt) b.xiso[(size_t)vox * b.n_iso + k] = nan;
            continue;
        }
        int steps_done = 0;
        const int status = bpp::solve<AT, true>(w, At, ldA, m, n, G, b.ldG, b.c.lam1, b.c.lam2, sqrt(ysq), b.lcap, Lg, b.full_start != 0, &steps_done, tid);
        if (status == kIterCap && tid == 0) atomicAdd(&b.c.status[ST_ITCAP], 1);
        if (status > kIterCap && tid == 0) { atomicAdd(&b.c.status[ST_GUARD], 1); b.c.status[ST_GUARDVOX] = vox * 8 + status; }
        // ---- x (exact zeros off the support) in atom order; SANDI: x *= norms first (models.pyx:1570-1571)
        double *xs = w.xo;                                        // (the single exchanges' point is done with)
        __syncthreads();
        for (int j = tid; j < n; j += nt) {
            double xj = (w.inP[j] && w.zat[j] > 0.0) ? w.zat[j] : 0.0;
            if (MODEL == 3) xj *= b.norms[j];
            xs[j] = xj;
            if (b.c.xdbg) b.c.xdbg[(size_t)vox * n + j] = xj;
        }
        __syncthreads();
        const double xj = tid < n ? xs[tid] : 0.0;               // (n <= 256: thread = atom)
        const int j = tid;
        if (MODEL == 2) {
            // models.pyx:1241-1256
            const int n_perp = b.n_a;
            const double x_sum = bpp::block_sum(xj, w.part, tid) + 1e-16;
            const double v = bpp::block_sum(j < n_perp ? xj : 0.0, w.part, tid) / x_sum;
            if (tid == 0) {
                double *e = b.est + (size_t)vox * b.n_maps;
                e[0] = v; e[1] = 1.0 - v;
                if (b.is_mouse) { e[2] = xs[n_perp] / x_sum; e[3] = (n_perp + 1 < n ? xs[n_perp + 1] : 0.0) / x_sum; }
            }
            if (b.xiso)
                for (int k = tid; k < b.n_iso; k += nt) b.xiso[(size_t)vox * b.n_iso + k] = xs[n_perp + k];
            if (b.ycorr) {
                // models.pyx:1264-1274: y - A[:, iso atoms] x_iso, clipped at 0
                for (int i = tid; i < m; i += nt) {
                    double fw = 0.0;
                    for (int k = n_perp; k < n; k++) fw += (double)At[(size_t)i * ldA + k] * xs[k];
                    const double yc = w.yv[i] - fw;
                    b.ycorr[(size_t)vox * m + i] = yc < 0.0 ? 0.0 : yc;
                }
            }
        } else if (MODEL == 3) {
            // models.pyx:1572-1612
            const int n_rs = b.n_a, n_in = b.n_b;
            const bool act = j < n, sph = act && j < n_rs, stk = act && j >= n_rs && j < n_rs + n_in, iso = act && j >= n_rs + n_in;
            const double x_sum = bpp::block_sum(xj, w.part, tid) + 1e-16;
            const double xsph = bpp::block_sum(sph ? xj : 0.0, w.part, tid), xstk = bpp::block_sum(stk ? xj : 0.0, w.part, tid);
            const double xiso = bpp::block_sum(iso ? xj : 0.0, w.part, tid);
            const double Rsoma = bpp::block_sum(sph ? b.Rs[j] * xj : 0.0, w.part, tid);
            const double Din = bpp::block_sum(stk ? b.d_in[j - n_rs] * xj : 0.0, w.part, tid);
            const double De = bpp::block_sum(iso ? b.d_isos[j - n_rs - n_in] * xj : 0.0, w.part, tid);
            if (tid == 0) {
                double *e = b.est + (size_t)vox * 6;
                e[0] = xsph / x_sum; e[1] = xstk / x_sum; e[2] = xiso / x_sum;
                e[3] = 1e6 * Rsoma / (xsph + 1e-16);
                e[4] = 1e3 * Din / (xstk + 1e-16);
                e[5] = 1e3 * De / (xiso + 1e-16);
            }
            // quirk kept (models.pyx:1571 then 1615): errors use the RESCALED x with the NORMALISED A -- a residual of its own
            if (b.c.flags & 3u) bpp::tile_residual(At, ldA, m, w.plist, w.shi[0], xs, true, w.yv, w.rv, tid);
        } else {
            // models.pyx:616-633
            const int n_rs = b.n_a, n_perp = b.n_b;
            const bool cyl = j < n_rs && j < n;
            double f1 = bpp::block_sum(cyl ? xj : 0.0, w.part, tid);
            const double f2 = bpp::block_sum((j >= n_rs && j < n_rs + n_perp && j < n) ? xj : 0.0, w.part, tid) + 1e-16;
            const double v = f1 / (f1 + f2 + 1e-16);
            f1 += 1e-16;
            double am = bpp::block_sum(cyl ? b.Rs[j] * xj : 0.0, w.part, tid);
            am = 1e6 * 2.0 * am / f1;
            const double d = (4.0 * v) / (3.14159265358979323846 * (am * am) + 1e-16);
            if (tid == 0) { double *e = b.est + (size_t)vox * 3; e[0] = v; e[1] = am; e[2] = d; }
        }
        if (b.c.flags & 3u) {
            double rr = 0.0;
            for (int i = tid; i < m; i += nt) rr += w.rv[i] * w.rv[i];
            const double rsq = bpp::block_sum(rr, w.part, tid);
            if (tid == 0) {
                if (b.rmse) b.rmse[vox] = sqrt(rsq / (double)m);
                if (b.nrmse) b.nrmse[vox] = (ysq > 1e-16) ? sqrt(rsq / ysq) : 0.0;
            }
        }
    }
}

template <typename AT, int MODEL>
int launch_enet_big(amx_ctx *ctx, const amx_lut *lut, EnetBigArgs &b, hipStream_t s, const SmallRoute &rt)
{
    const int m = b.c.nS, n = b.c.n_atoms;
    b.gram = lut->gram; b.ldG = lut->ldG; b.ndirs = lut->ndirs;
    b.full_start = (b.c.lam1 == 0.0 && b.c.lam2 >= 1e-2) ? 1 : 0;
    const size_t vec = bpp::vec_bytes(m, n);      // (the route has seen that they fit, and that the dictionary has its Gram table)
    int lcap = 0;
    while (lcap < n && vec + ((size_t)(lcap + 1) * (lcap + 2) / 2) * sizeof(double) <= kLdsPerCU) lcap++;
    b.lcap = lcap;
    const size_t lds = vec + ((size_t)lcap * (lcap + 1) / 2) * sizeof(double);
    // workgroups: as many as the LDS lets a CU hold (at most 4: a wavefront per SIMD each, 112 .. 118 registers), over every CU; never more than voxels
    int per_cu = (int)(kLdsPerCU / lds);
    per_cu = (per_cu < 1 || lcap < n) ? 1 : (per_cu > 4 ? 4 : per_cu);      // (the global factor blocks: one per CU)
    int64_t grid = (int64_t)ctx->n_cu * per_cu;
    if (grid > b.n_vox) grid = b.n_vox;
    int rc;
    if (lcap < n) {
        // (one set of factor blocks per workspace set: the batches of a host-buffer call alternate between two streams)
        const size_t blk = (size_t)n * (n + 1) / 2;
        if ((rc = amx_ensure(ctx, ctx->big, 2 * (size_t)ctx->n_cu * blk * sizeof(double)))) return rc;
        b.Lg = (double *)ctx->big.p + (size_t)ctx->work_idx * ctx->n_cu * blk;
    }
    rec(ctx, 4, s);
    if ((rc = launch_lds(ctx, k_enet_big<AT, MODEL>, dim3((unsigned)grid), dim3(kEbThreads), lds, s, b))) return rc;
    amx_note(ctx, rt.launch[0]);
    AMX_TRACE(ctx, s, "dictionaries of 65 .. 256 atoms (block principal pivoting, workgroup per voxel)");
    rec(ctx, 5, s);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

void common_args(EnetBigArgs &b, const FitCommon &c, const Plan *pl, int ndirs, int64_t n)
{
    memset(&b, 0, sizeof b);
    b.c = c;
    b.n_vox = (int)n;
    if (pl) b.count = pl->dir_start + ndirs;                      // k_plan: the voxels it bucketed
    else { b.c.perm = nullptr; b.c.lutidx = nullptr; }
}

}  // namespace

int amx_launch_enet_big(amx_ctx *ctx, const amx_lut *lut, const FwArgs &a, const Plan &pl, int64_t n, hipStream_t s, const SmallRoute &rt)
{
    EnetBigArgs b;
    common_args(b, a.c, &pl, lut->ndirs, n);
    b.est = a.est; b.rmse = a.rmse; b.nrmse = a.nrmse; b.n_maps = a.n_maps;
    b.n_a = a.n_perp; b.n_iso = a.n_iso; b.is_mouse = a.is_mouse; b.ycorr = a.ycorr; b.xiso = a.xiso;
    return launch_enet_big<float, 2>(ctx, lut, b, s, rt);
}

int amx_launch_enet_big(amx_ctx *ctx, const amx_lut *lut, const SandiArgs &a, int64_t n, hipStream_t s, const SmallRoute &rt)
{
    EnetBigArgs b;
    common_args(b, a.c, nullptr, 1, n);                           // (one dictionary: the voxels in order)
    b.est = a.est; b.rmse = a.rmse; b.nrmse = a.nrmse; b.n_maps = 6;
    b.n_a = a.n_rs; b.n_b = a.n_in; b.n_iso = a.n_iso;
    b.norms = a.norms; b.Rs = a.Rs; b.d_in = a.d_in; b.d_isos = a.d_isos;
    return launch_enet_big<double, 3>(ctx, lut, b, s, rt);
}

int amx_launch_enet_big(amx_ctx *ctx, const amx_lut *lut, const CzbArgs &a, const Plan &pl, int64_t n, hipStream_t s, const SmallRoute &rt)
{
    EnetBigArgs b;
    common_args(b, a.c, &pl, lut->ndirs, n);
    b.est = a.est; b.rmse = a.rmse; b.nrmse = a.nrmse; b.n_maps = 3;
    b.n_a = a.n_rs; b.n_b = a.n_perp; b.Rs = a.Rs;
    return launch_enet_big<float, 4>(ctx, lut, b, s, rt);
}

// G_d of every orientation of a dictionary of more than 64 atoms into lut->gram, on the null stream (the upload's)
int amx_build_big_gram(amx_ctx *ctx, amx_lut *lut)
{
    const int n = lut->n_atoms;
    lut->ldG = (n + 3) & ~3;
    const size_t gbytes = (size_t)lut->ndirs * n * lut->ldG * sizeof(double);
    if (hipMalloc((void **)&lut->gram, gbytes) != hipSuccess) { (void)hipGetLastError(); lut->gram = nullptr; return amx_bad(ctx, "dictionary upload: out of device memory for the Gram tables"); }
    const dim3 grid((unsigned)((size_t)lut->ndirs * n));
    if (lut->model == 3) hipLaunchKernelGGL(k_big_gram<double>, grid, dim3(256), 0, nullptr, (const double *)lut->tiles, lut->nS, n, lut->ldA, lut->tile_stride, lut->ldG, lut->gram);
    else hipLaunchKernelGGL(k_big_gram<float>, grid, dim3(256), 0, nullptr, (const float *)lut->tiles, lut->nS, n, lut->ldA, lut->tile_stride, lut->ldG, lut->gram);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}
