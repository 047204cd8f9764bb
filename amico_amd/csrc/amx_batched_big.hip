// amx_batched_big.hip -- the batched nnls / lasso entry points on a dictionary marked DENSE (amx_dict_set_dense): supports of ANY size.
//
// The wavefront-per-voxel kernels of amx_batched.hip hold 16 passive atoms (main pass) and 48 (re-run pass); what does not fit there either is
// AMX_E_OVERFLOW on an ordinary dictionary.  On a dense one the re-run pass writes those voxels to a list of its own (launch_pair, big_after) and
// k_batched_big takes them from it, one WORKGROUP of 256 threads per voxel (the layout of k_noddi_lasso_big, amx_big.hip):
//     min_{x >= 0} 1/2 ||y - A x||^2 + lambda1 sum(x) + lambda2/2 ||x||^2              (nnls: lambda1 = lambda2 = 0)
// in Gram space, H = G_d + lambda2 I from the dictionary's Gram table (k_dict_gram, made once by amx_dict_set_dense), c = A_d'y - lambda1 from the
// fp64 tile where it lies.  The solver is amx_bpp.hpp's: block principal pivoting from the kStart best single atoms on a packed Cholesky factor,
// thresholds relative to the voxel, the rank guard with Lawson-Hanson exchanges, the check on the true problem (rnorm = ||r|| of that check);
// its loop is shared with k_enet_big (amx_enet_big.hip).
// The kernel takes its voxels from the device list and its device count alone (never perm[0 .. n): ADVICE.md).
#include "amx_launch.hpp"
#include "amx_bpp.hpp"
using namespace amx;

namespace {

struct BigBatchedArgs {
    BatchedArgs a;
    const double *gram;           // [n_dicts][n][ldG]
    int ldG;
    const int *list;              // voxel numbers
    const int *count;             // their number (device)
    int lcap;                     // largest passive set whose packed factor lies in LDS
    double *Lg;                   // global factor blocks [gridDim.x][n (n + 1) / 2], or null (n <= lcap)
};

constexpr int kBbThreads = bpp::kThreads, kBbGrid = 256;

__global__ void __launch_bounds__(kBbThreads) k_batched_big(const BigBatchedArgs b)
{
    const BatchedArgs &a = b.a;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_bb[];
    const int m = a.c.nS, ldA = a.c.ldA, n = a.c.n_atoms;
    const bpp::Work w = bpp::carve(smem_bb, m, n);
    double *Lg = b.Lg ? b.Lg + (size_t)blockIdx.x * ((size_t)n * (n + 1) / 2) : w.Ll;
    const int tid = threadIdx.x, nt = kBbThreads;
    const double *tiles = reinterpret_cast<const double *>(a.c.tiles);
    const int cnt = *b.count;

    for (int it = blockIdx.x; it < cnt; it += gridDim.x) {
        const int vox = b.list[it];
        const int dic = a.c.lutidx[vox];
        const double *At = tiles + (size_t)dic * a.c.tile_stride;
        const double *G = b.gram + (size_t)dic * n * b.ldG;
        double *dst = a.x + (size_t)vox * n;
        __syncthreads();
        if (tid < 16) w.shi[tid] = 0;
        __syncthreads();
        double yy = 0.0;
        for (int i = tid; i < m; i += nt) {
            const double yi = a.c.y[(size_t)vox * m + i];
            if (!(fabs(yi) <= 1.79769313486231570e308)) w.shi[4] = 1;
            w.yv[i] = yi; w.rv[i] = yi;
            yy += yi * yi;
        }
        const double ynorm = sqrt(bpp::block_sum(yy, w.part, tid));
        if (w.shi[4]) {                                           // non-finite signal: NaN out, like batched_voxel
            for (int j = tid; j < n; j += nt) dst[j] = __builtin_nan("");
            if (tid == 0 && a.rnorm) a.rnorm[vox] = __builtin_nan("");
            continue;
        }
        int steps_done = 0;
        const int status = bpp::solve(w, At, ldA, m, n, G, b.ldG, a.c.lam1, a.c.lam2, ynorm, b.lcap, Lg, false, &steps_done, tid);
        // ---- out: the row of x (exact zeros off the support), ||r|| of the true residual
        if (status == kIterCap && tid == 0) atomicAdd(&a.c.status[ST_ITCAP], 1);
        if (status > kIterCap && tid == 0) { atomicAdd(&a.c.status[ST_GUARD], 1); a.c.status[ST_GUARDVOX] = vox * 8 + status; }
        for (int j = tid; j < n; j += nt) dst[j] = (w.inP[j] && w.zat[j] > 0.0) ? w.zat[j] : 0.0;
        if (a.rnorm) {
            double rr = 0.0;
            for (int i = tid; i < m; i += nt) rr += w.rv[i] * w.rv[i];
            rr = bpp::block_sum(rr, w.part, tid);
            if (tid == 0) a.rnorm[vox] = sqrt(rr);
        }
        if (tid == 0) { atomicAdd(&a.c.status[ST_DENSE], 1); atomicAdd(&a.c.status[ST_DENSE + 1], steps_done); }
    }
}

size_t bb_vec_bytes(int m, int n) { return bpp::vec_bytes(m, n); }

// G_d = A_d'A_d, one workgroup per (dictionary, row): the row's atom is read by every thread, the other atom across the threads
__global__ void __launch_bounds__(256) k_dict_gram(const double *__restrict__ tiles, int m, int n, int ldA, int tile_stride, int ldG, double *__restrict__ G)
{
    const int d = blockIdx.x / n, j = blockIdx.x % n, k = threadIdx.x;
    if (k >= ldG) return;
    const double *At = tiles + (size_t)d * tile_stride;
    double acc = 0.0;
    if (k < n)
        for (int i = 0; i < m; i++) acc += At[(size_t)i * ldA + j] * At[(size_t)i * ldA + k];
    G[((size_t)d * n + j) * ldG + k] = acc;
}

}  // namespace

// the voxels the 48-atom re-run pass of a dense dictionary wrote to list 6 (launch_pair, big_after): one launch, whatever their number
int amx_launch_batched_big(amx_ctx *ctx, const BatchedArgs &a, const amx_dict *dict, const Plan &pl, hipStream_t s)
{
    BigBatchedArgs b;
    memset(&b, 0, sizeof b);
    b.a = a; b.gram = dict->gram; b.ldG = dict->ldG;
    b.list = pl.ovf_list + (size_t)6 * pl.n; b.count = pl.ovf_count + 10;
    const int m = a.c.nS, n = a.c.n_atoms;
    const size_t vec = bb_vec_bytes(m, n);
    if (vec > kLdsPerCU) { ctx->err = "k_batched_big: the dictionary's vectors do not fit the LDS"; return AMX_E_BADARG; }
    int lcap = 0;
    while (lcap < n && vec + ((size_t)(lcap + 1) * (lcap + 2) / 2) * sizeof(double) <= kLdsPerCU) lcap++;
    b.lcap = lcap;
    int rc;
    if (lcap < n) {
        if ((rc = amx_ensure(ctx, ctx->big, (size_t)kBbGrid * ((size_t)n * (n + 1) / 2) * sizeof(double)))) return rc;
        b.Lg = (double *)ctx->big.p;
    }
    const size_t lds = vec + ((size_t)lcap * (lcap + 1) / 2) * sizeof(double);
    rec(ctx, 4, s);
    if ((rc = launch_lds(ctx, k_batched_big, dim3(kBbGrid), dim3(kBbThreads), lds, s, b))) return rc;
    amx_note(ctx, "k_batched_big (dense dictionary: supports beyond 48 atoms)");
    AMX_TRACE(ctx, s, "batched solvers, any support size (block principal pivoting, workgroup per voxel)");
    rec(ctx, 5, s);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

// G_d of every dictionary of `dict` into dict->gram (allocated by the caller: amx_dict_set_dense), on the null stream
int amx_build_dict_gram(amx_ctx *ctx, const amx_dict *dict)
{
    hipLaunchKernelGGL(k_dict_gram, dim3((unsigned)((size_t)dict->n_dicts * dict->n)), dim3(256), 0, nullptr, dict->tiles, dict->m, dict->n, dict->ldA,
                       dict->tile_stride, dict->ldG, dict->gram);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(nullptr));
    return AMX_OK;
}
