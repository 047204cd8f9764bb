// amx_plan.hip -- home of the amx_prep.hpp kernels (a header of plain kernels: one unit may include it) and of every launch of them: the
// per-call plan (voxels bucketed by orientation, chunks, workspace), the counters, the widening, amx_dir_to_lut_idx.
#include "amx_host.hpp"
#include "amx_prep.hpp"

using namespace amx;

int make_plan(amx_ctx *ctx, int64_t n, int ndirs, Plan &pl, const NoddiRoute *seeds, int table_rows, int blocks_chunk)
{
    int rc;
    const int max_chunks = (int)(n / kChunk) + ndirs + 1;
    pl.n = (size_t)n;
    if (seeds) {
        // the second plan: its chunk, the wavefronts and builds of the lane kernels are the route's (amx_noddi_route.hpp)
        pl.seed_chunk = seeds->seed_chunk; pl.max_schunks = seeds->max_schunks;
        pl.seed_waves = seeds->seed_waves; pl.seed1_waves = seeds->seed1_waves; pl.seed2_waves = seeds->seed2_waves;
        pl.seed_occ2 = seeds->seed_occ2; pl.seed2_occ2 = seeds->seed2_occ2;
        if ((rc = amx_ensure(ctx, ctx->schunks, (size_t)pl.max_schunks * sizeof(Chunk)))) return rc;
        if ((rc = amx_ensure(ctx, ctx->ytil, (size_t)n * amx::kSeedKD * sizeof(double)))) return rc;
        if ((rc = amx_ensure(ctx, ctx->seeds, (size_t)n * sizeof(unsigned long long)))) return rc;
        // the A'y table of all voxels, and the compact table of the voxels whose stage-2 signal clips (sized for all of them: a
        // dictionary whose b0 rows are not ones sends every voxel there), the clipped lists / counts / slots of k_s2_prep
        if ((rc = amx_ensure(ctx, ctx->cgemm, ((size_t)n / 64 + ndirs + 1) * table_rows * 64 * sizeof(double)))) return rc;
        if ((rc = amx_ensure(ctx, ctx->cgemm2, ((size_t)n / 64 + ndirs + 1) * table_rows * 64 * sizeof(double)))) return rc;
        if ((rc = amx_ensure(ctx, ctx->clip, ((size_t)2 * n + pl.max_schunks + 64) * sizeof(int)))) return rc;
        if ((rc = amx_ensure(ctx, ctx->feed, (size_t)(kFeedSets + kZCounts) * (pl.max_schunks + 8) * sizeof(int)))) return rc;      // chunk counters of the kernels that share their chunks (SeedFeed, BlockFeed) + the list counts of every pass (Plan::zcount)
        if ((rc = amx_ensure(ctx, ctx->done, (size_t)n + 64))) return rc;
        if ((rc = amx_ensure(ctx, ctx->rlist, 4 * amx_rlist_half(pl) * sizeof(int)))) return rc;      // (two halves per stage's certificate passes; a forked fit's stage 3 takes the third and fourth)
        if ((rc = amx_ensure(ctx, ctx->ytil2, (size_t)n * amx::kSeedKD * sizeof(double)))) return rc;
        if ((rc = amx_ensure(ctx, ctx->seeds2, (size_t)n * 4 * sizeof(unsigned long long)))) return rc;
        pl.schunks = (Chunk *)ctx->schunks.p;
        pl.feed = (int *)ctx->feed.p;
    }
    if (!seeds && blocks_chunk > 0) {
        // second plan only (chunks of whole 64-voxel blocks) + a block-wise table of table_rows rows: CylinderZeppelinBall's fast path
        pl.seed_chunk = blocks_chunk;
        pl.max_schunks = (int)(n / blocks_chunk) + ndirs + 1;
        if ((rc = amx_ensure(ctx, ctx->schunks, (size_t)pl.max_schunks * sizeof(Chunk)))) return rc;
        if ((rc = amx_ensure(ctx, ctx->cgemm, ((size_t)n / 64 + ndirs + 1) * table_rows * 64 * sizeof(double)))) return rc;
        pl.schunks = (Chunk *)ctx->schunks.p;
    }
    if ((rc = amx_ensure(ctx, ctx->lutidx, n * sizeof(int)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->perm, n * sizeof(int)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->counts, (size_t)(ndirs + 1) * sizeof(int)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->dir_start, (size_t)(ndirs + 1) * sizeof(int)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->cursor, (size_t)(ndirs + 1) * sizeof(int)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->chunks, (size_t)max_chunks * sizeof(Chunk)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->misc, 64 * sizeof(int)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->ovf, (size_t)7 * n * sizeof(int)))) return rc;      // (lists 0 .. 2: the stages' overflow, 3: second level; 4, 5: the same for a forked fit's side stream; 6: what k_noddi_lasso_big takes; amx_launch.hpp)
    pl.lutidx = (int *)ctx->lutidx.p; pl.perm = (int *)ctx->perm.p; pl.counts = (int *)ctx->counts.p;
    pl.dir_start = (int *)ctx->dir_start.p; pl.cursor = (int *)ctx->cursor.p;
    pl.chunks = (Chunk *)ctx->chunks.p; pl.n_chunks = (int *)ctx->misc.p;
    pl.ovf_count = (int *)ctx->misc.p + 4; pl.ovf_list = (int *)ctx->ovf.p;
    pl.max_chunks = max_chunks;
    pl.n = (size_t)n;
    return AMX_OK;
}

int enqueue_bucketing(amx_ctx *ctx, const amx_lut *lut, const double *d_dirs, int64_t n, Plan &pl, hipStream_t s, int chunk,
                      double *zero_rows, int zero_cols, double *zero_rows2, int zero_cols2)
{
    // (four launches: the counters cleared in one, the chunk order in k_plan's tail; they were three memsets and five kernels --
    //  ~11 us a node in a small call, profiles/r06_launch_nodes.txt)
    const int n_feed = pl.feed ? (kFeedSets + kZCounts) * (pl.max_schunks + 8) : 0;
    hipLaunchKernelGGL(k_clear3, dim3(n_feed > 4096 ? 8 : 1), dim3(1024), 0, s, pl.counts, lut->ndirs + 1, (int *)ctx->misc.p, 64, pl.feed, n_feed);
    const int span = prep_span(n);
    const int nb = (int)((n + span - 1) / span);
    const int use_lds = lut->ndirs <= 8192 ? 1 : 0;          // LDS histograms: 2 * ndirs ints
    hipLaunchKernelGGL(k_dir_to_lut, dim3(nb), dim3(1024), use_lds ? (size_t)lut->ndirs * sizeof(int) : 0, s, d_dirs,
                       (int)n, lut->htable, lut->ndirs, pl.lutidx, pl.counts, ctx->status_d, use_lds, (int)ctx->batch.base, span, zero_rows, zero_cols, zero_rows2, zero_cols2);
    AMX_TRACE(ctx, s, "k_dir_to_lut");
    hipLaunchKernelGGL(k_plan, dim3(1), dim3(1024), 0, s, pl.counts, lut->ndirs, chunk, pl.dir_start,
                       pl.cursor, pl.chunks, pl.n_chunks, pl.schunks ? pl.seed_chunk : 0, pl.schunks, (pl.schunks && !ctx->opt_no_chunk_order) ? 1 : 0);
    AMX_TRACE(ctx, s, "k_plan");
    hipLaunchKernelGGL(k_bucket, dim3(nb), dim3(1024), use_lds ? (size_t)2 * lut->ndirs * sizeof(int) : 0, s, pl.lutidx,
                       (int)n, lut->ndirs, pl.dir_start, pl.cursor, pl.perm, use_lds, span);
    AMX_TRACE(ctx, s, "k_bucket");
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

namespace {

// per-call counters (misc, cleared by the next call) -> status words that accumulate until amx_sync_status
__global__ void k_fold_counters(const int *misc, int *status)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        atomicAdd(&status[ST_RERUN], misc[4] + misc[5] + misc[6] + misc[7]);      // (two batches may fold concurrently: fit_host)
        atomicAdd(&status[ST_OVERFLOW], misc[12] + misc[13]);
    }
}

// float32 signals (the image dtype of the reference, core.py:136) -> the float64 rows the solvers read: exact
__global__ void k_widen(const float *__restrict__ src, double *__restrict__ dst, size_t n)
{
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    // (16-byte loads only from a 16-byte aligned source: a row slice of a float32 tensor may start at any multiple of 4 bytes)
    if (i0 + 3 < n && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const float4 v = *reinterpret_cast<const float4 *>(src + i0);
        dst[i0] = (double)v.x; dst[i0 + 1] = (double)v.y; dst[i0 + 2] = (double)v.z; dst[i0 + 3] = (double)v.w;
    } else {
        for (size_t i = i0; i < n; i++) dst[i] = (double)src[i];
    }
}

}  // namespace

// histogram of the caller's dictionary indices (+ range check: the first bad voxel is reported like a bad direction)
__global__ void k_idx_hist(const int *__restrict__ idx, int n, int n_dicts, int *__restrict__ lutidx, int *__restrict__ counts, int *__restrict__ status)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    int d = idx ? idx[v] : 0;
    if (d < 0 || d >= n_dicts) {
        // first bad voxel and ITS index in one 64-bit atomic (two plain stores after an atomicMin on the voxel alone could pair the
        // smallest voxel with another voxel's index); k_fold_counters unpacks it into ST_ERRVOX / ST_II1
        atomicMin(reinterpret_cast<unsigned long long *>(status + ST_ERRPACK), ((unsigned long long)(unsigned)v << 32) | (unsigned)d);
        status[ST_II2] = n_dicts; status[ST_ERRKIND] = 1;      // (the same values from every lane)
        d = -1;
    } else {
        atomicAdd(&counts[d], 1);
    }
    lutidx[v] = d;
}

void fold_counters(amx_ctx *ctx, hipStream_t s)
{
    hipLaunchKernelGGL(k_fold_counters, dim3(1), dim3(64), 0, s, (const int *)ctx->misc.p, ctx->status_d);
}

void widen_on_device(const float *d_y32, double *dst, size_t nel, hipStream_t s)
{
    hipLaunchKernelGGL(k_widen, dim3((unsigned)((nel / 4 + 256) / 256)), dim3(256), 0, s, d_y32, dst, nel);
}

int enqueue_index_bucketing(amx_ctx *ctx, const int32_t *d_idx, int n_dicts, int64_t n_vox, Plan &pl, hipStream_t s)
{
    HIPCHK(ctx, hipMemsetAsync(pl.counts, 0, (size_t)(n_dicts + 1) * sizeof(int), s));
    HIPCHK(ctx, hipMemsetAsync(ctx->misc.p, 0, 64 * sizeof(int), s));
    hipLaunchKernelGGL(k_idx_hist, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, s, (const int *)d_idx, (int)n_vox, n_dicts, pl.lutidx, pl.counts, ctx->status_d);
    hipLaunchKernelGGL(k_plan, dim3(1), dim3(1024), 0, s, pl.counts, n_dicts, kChunk, pl.dir_start, pl.cursor, pl.chunks, pl.n_chunks, 0, (Chunk *)nullptr, 0);
    const int nb = (int)((n_vox + kPrepSpan - 1) / kPrepSpan);
    const int use_lds = n_dicts <= 8192 ? 1 : 0;
    hipLaunchKernelGGL(k_bucket, dim3(nb), dim3(1024), use_lds ? (size_t)2 * n_dicts * sizeof(int) : 0, s, pl.lutidx, (int)n_vox, n_dicts,
                       pl.dir_start, pl.cursor, pl.perm, use_lds, kPrepSpan);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

int enqueue_linear_plan(amx_ctx *ctx, int64_t n_vox, Plan &pl, hipStream_t s)
{
    HIPCHK(ctx, hipMemsetAsync(ctx->misc.p, 0, 64 * sizeof(int), s));
    const int nb = (int)((n_vox + 255) / 256);
    hipLaunchKernelGGL(k_plan_linear, dim3(nb), dim3(256), 0, s, (int)n_vox, kChunk, pl.chunks, pl.n_chunks, pl.perm);
    return AMX_OK;
}

// a profiled call starts with no event pair valid: amx_last_kernel_ms of a group this call does not run is an error, not the
// timing of an earlier call (the dti / prep / lut entry points record slot 4 only and clear it themselves)
void clear_events(amx_ctx *ctx)
{
    if (ctx->profiling) for (int k = 0; k < kEv; k++) ctx->ev_valid[k] = false;
}

// Device-pointer entry points: the fit is only ENQUEUED when the call returns, so the callback is a host function on the
// stream (hipLaunchHostFunc) -- it runs on a runtime thread once everything enqueued before it has finished.
struct ProgressTick { amx_ctx *ctx; int64_t done, total; };
static void progress_host_fn(void *p)
{
    ProgressTick *t = static_cast<ProgressTick *>(p);
    if (t->ctx->progress) t->ctx->progress(t->done, t->total, t->ctx->progress_user);
    delete t;
}
void progress_tick(amx_ctx *ctx, hipStream_t s, int64_t done, int64_t total)
{
    if (!ctx->progress || ctx->batch.host) return;
    ProgressTick *t = new ProgressTick{ctx, done, total};
    if (hipLaunchHostFunc(s, progress_host_fn, t) != hipSuccess) { (void)hipGetLastError(); delete t; }
}

// the LUT index of every voxel alone, into a buffer of the caller's (amx_predict.hip): no histogram, no plan; a direction out of bounds
// gives -1 and is reported through the status words like the fit reports it
int enqueue_dir_to_lut(amx_ctx *ctx, const amx_lut *lut, const double *d_dirs, int64_t n, int *d_idx, hipStream_t s)
{
    if (!lut->htable) return amx_bad(ctx, "dictionary has no hash table");
    const int span = prep_span(n);
    hipLaunchKernelGGL(k_dir_to_lut, dim3((unsigned)((n + span - 1) / span)), dim3(1024), 0, s, d_dirs, (int)n, lut->htable, lut->ndirs, d_idx,
                       (int *)nullptr, ctx->status_d, 0, 0, span, (double *)nullptr, 0, (double *)nullptr, 0);
    HIPCHK(ctx, hipGetLastError());
    return AMX_OK;
}

// (here, beside the other launches of k_dir_to_lut)
extern "C" int amx_dir_to_lut_idx(amx_ctx *ctx, const amx_lut *lut, const double *dirs, int64_t n, int32_t *out_idx)
{
    if (!ctx) return AMX_E_BADARG;
    if (!lut || !lut->htable) return amx_bad(ctx, "amx_dir_to_lut_idx: dictionary has no hash table");
    if (n == 0) return AMX_OK;
    if (n < 0 || n > INT_MAX / 4 || !dirs || !out_idx) return amx_bad(ctx, "amx_dir_to_lut_idx: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    AMX_H2D(ctx->hdirs, dirs, (size_t)n * 3 * sizeof(double))
    if ((rc = amx_ensure(ctx, ctx->lutidx, (size_t)n * sizeof(int)))) return rc;
    hipLaunchKernelGGL(k_dir_to_lut, dim3((unsigned)((n + kPrepSpan - 1) / kPrepSpan)), dim3(1024), 0, nullptr,
                       (const double *)ctx->hdirs.p, (int)n, lut->htable, lut->ndirs, (int *)ctx->lutidx.p, (int *)nullptr,
                       ctx->status_d, 0, 0, kPrepSpan, (double *)nullptr, 0, (double *)nullptr, 0);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_idx, ctx->lutidx.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, nullptr));
    return amx_sync_status(ctx, nullptr);
}
