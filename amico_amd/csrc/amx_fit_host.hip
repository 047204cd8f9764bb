// amx_fit_host.hip -- the four model fits on host buffers: batches, the float32 transport, results home (fit_host), and their C entry points.
#include "amx_host.hpp"
#include <algorithm>
#include <chrono>
#include <thread>

using namespace amx;

namespace {

void progress(amx_ctx *ctx, int64_t done, int64_t total)
{
    if (ctx->progress) ctx->progress(done, total, ctx->progress_user);
}

// The host threads + pinned ring of the float32 transport (amx_stage.hpp).  The threads stay on the NUMA node the DEVICE hangs on, one stripe of
// physical cores each: the pinned ring they write lives there and the copies leave from there; the caller's buffer is read across the socket
// link if it lives on the other node.  Measured on the two-socket box, host_trace.py and bench.py, two processes each: 12.6 - 12.9 ms per 1 M
// voxels in all four; on the calling thread's node 15.5 - 19 ms when that is the far socket (AMX_HOST_PIN = gpu | caller | 0: diagnosis;
// profiles/r05c_host_transport.txt, section 8)
amx_stage::Pool *make_stage_pool(amx_ctx *ctx)
{
    const unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)ctx->opt_host_threads;
    if (hw >= 2 && nt > (int)(hw / 2)) nt = (int)(hw / 2);
    int node = -1;
    const bool pin_gpu = ctx->opt_host_pin == 'g', pin_caller = ctx->opt_host_pin == 'c';
    if (pin_gpu) node = amx_stage::device_node(ctx->device);
    if (pin_caller || (pin_gpu && node < 0)) {
        const int cpu = sched_getcpu();
        cpu_set_t cs;
        for (int nd = 0; nd < 16 && cpu >= 0; nd++)
            if (amx_stage::node_cpus(nd, &cs) && CPU_ISSET(cpu, &cs)) { node = nd; break; }
    }
    // the other devices of that node have pools of their own (this process's other contexts, or other ranks): disjoint shares
    int sib_i = 0, sib_n = 1;
    if (ctx->opt_host_siblings[1] >= 1 && ctx->opt_host_siblings[0] >= 0) { sib_i = (int)ctx->opt_host_siblings[0]; sib_n = (int)ctx->opt_host_siblings[1]; }   // AMX_HOST_SIBLINGS=i/n forces
    else if (pin_gpu) amx_stage::device_siblings(ctx->device, node, (int)ctx->opt_local_rank, (int)ctx->opt_local_world, &sib_i, &sib_n);
    return amx_stage::Pool::create(nt < 1 ? 1 : nt, node, sib_i, sib_n, (char)ctx->opt_host_pin_cores);
}

// Host buffers in, host buffers out, for all three models and both signal dtypes (float64 = evaluation.y of the
// reference; float32 = the dtype the image has before core.py:451 casts it -- lossless, half the PCIe bytes).
// Large inputs travel in batches: while the GPU fits batches c-1 and c-2 (on the two non-blocking streams of the
// context, each with its own workspace set) the blocking host-to-device copy of batch c is already running, so the PCIe
// time hides behind the solver instead of preceding it.  Three signal buffers; results leave in one copy per output at the end.  The
// progress callback (amx_set_progress; models.pyx:28-43, 981 keep a per-thread counter for the same purpose) is called as batches complete.
// (largest batch; measured on 1 M NODDI voxels: 131072 -> 38.3 ms, 262144 -> 37.2 ms, 393216 -> 36.3 ms per call)

struct HostOut { void *dst; DevBuf *buf; size_t cols; bool on; };

// One host-buffer call of any model: `call` holds the caller's HOST pointers; every batch is enqueued through amx_fit_dev with
// device pointers into the staging buffers in their place.  native32: the model's kernels read float32 signals in place (no k_widen pass).
template <typename T>
int fit_host(amx_ctx *ctx, const FitSpec &m, const FitCall &call, const T *y, bool native32_model, HostOut (&outs)[4])
{
    const double *dirs = call.dirs; const int64_t n_vox = call.n; const int nS = call.lut->nS;
    int rc;
    const int64_t kHostBatch = ctx->opt_host_batch;
    constexpr bool kF32 = sizeof(T) == 4;
    const bool pipelined = n_vox >= ctx->opt_host_pipeline_from && !ctx->opt_host_one_shot;
    constexpr int kBufs = 3;                      // staging buffers: batch c uploads while c-1 and c-2 are being solved
    const int64_t cap = pipelined ? kBufs * kHostBatch : n_vox;
    // float64 signals that are float32 values (evaluation.y always is: core.py:136, 451) cross the link as float32 (amx_stage.hpp)
    constexpr size_t kNarrowFrom = 2u << 20;      // elements of a batch from which the host threads are worth waking (16 MB: 0.3 ms of link)
    bool narrow = false;
    if (!kF32 && !ctx->opt_host_no_narrow && !ctx->stage_failed && (size_t)n_vox * nS >= kNarrowFrom) {
        if (!ctx->stage) {
            if (ctx->stage_thread.joinable()) { ctx->stage_thread.join(); ctx->stage = ctx->stage_bg; ctx->stage_bg = nullptr; }      // made beside the dictionary upload
            if (!ctx->stage) ctx->stage = make_stage_pool(ctx);
            if (!ctx->stage) ctx->stage_failed = true;
        }
        narrow = ctx->stage != nullptr;
    }
    ctx->host_narrowed = 0;
    // (a model whose kernels read float32 signals in place -- NODDI -- needs the float64 staging buffer only for a batch that
    //  could not travel as float32: made when that happens.  934 MB less to allocate in a process's first call, no k_widen pass per batch)
    const bool native32 = native32_model && !ctx->opt_host_no_native32;
    if (!(native32 && (kF32 || narrow)) && (rc = amx_ensure(ctx, ctx->hy, (size_t)cap * nS * sizeof(double)))) return rc;
    if ((kF32 || narrow) && (rc = amx_ensure(ctx, ctx->hy32, (size_t)cap * nS * sizeof(float)))) return rc;
    if (dirs && (rc = amx_ensure(ctx, ctx->hdirs, (size_t)cap * 3 * sizeof(double)))) return rc;
    for (HostOut &o : outs)
        if (o.on && (rc = amx_ensure(ctx, *o.buf, (size_t)n_vox * o.cols * sizeof(double)))) return rc;
    if (!ctx->up_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->up_ev, hipEventDisableTiming));
    if (!ctx->hs) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->hs, hipStreamNonBlocking));
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->hs2, hipStreamNonBlocking));
        for (hipEvent_t &e : ctx->hev) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIPCHK(ctx, hipStreamSynchronize(nullptr));                      // earlier default-stream work on these buffers
    // (the event pairs of a profiled call would be overwritten batch by batch; whatever way the call ends, profiling is as it was, and the next
    //  call on this ctx is nobody's batch)
    struct CallScope { amx_ctx *c; int profiling; ~CallScope() { c->profiling = profiling; c->batch = Batch(); } } call_scope{ctx, ctx->profiling};
    if (pipelined) ctx->profiling = 0;
    // (a shard of a larger call -- amx_set_call_voxels: one of several contexts that share a fit -- takes the paths the whole call's size asks for,
    //  as the batches of one call do: every context settles its voxels with the arithmetic the single-context call would use)
    const int64_t call_vox = ctx->call_total_vox > n_vox ? ctx->call_total_vox : n_vox;
    // Batch c runs on stream c & 1 with workspace set c & 1: the kernels of consecutive batches overlap, so the idle tail
    // of every launch (and the one-wavefront re-run kernels) is filled by the other batch instead of adding up six times.
    const bool two_streams = pipelined;
    hipStream_t s = pipelined ? ctx->hs : nullptr;
    int64_t off = 0, done_before[kBufs] = {0, 0, 0};         // voxels complete once the event of that buffer has fired
    // AMX_HOST_TRACE=1 (diagnosis): wall-clock timeline of the call on stderr -- per batch the wait for its buffer, its copy, its enqueue
    const bool trace = ctx->opt_host_trace;
    auto wall = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tr0 = trace ? wall() : 0.0;
    int64_t reported = 0;                                    // progress is reported once per batch, in order
    auto report = [&](int64_t v) { if (v > reported) { progress(ctx, v, n_vox); reported = v; } };
    auto batch_cnt = [&](int c, int64_t at) -> int64_t {
        const int64_t rem = n_vox - at, ramp = ctx->opt_host_ramp;
        const int64_t parts = (rem + kHostBatch - 1) / kHostBatch;
        return !pipelined ? n_vox : ((c < 1 && ramp > 0 && rem > 3 * ramp) ? ramp : (rem + parts - 1) / parts);
    };
    // the call's batches are known up front, and with them the chunks the host threads narrow ahead of the copies (amx_stage.hpp)
    std::vector<amx_stage::Chunk> chunks;
    std::vector<int> first_chunk;                  // of batch c
    if (narrow) {
        int64_t at = 0;
        for (int c = 0; at < n_vox; c++) {
            const int64_t cnt = batch_cnt(c, at);
            const size_t nel = (size_t)cnt * nS;
            if (nel < kNarrowFrom) { narrow = false; break; }         // (a batch too small to be worth it: SANDI's six values per voxel)
            first_chunk.push_back((int)chunks.size());
            for (size_t o = 0; o < nel; o += amx_stage::Pool::kChunkEl)
                chunks.push_back({(size_t)at * nS + o, nel - o < amx_stage::Pool::kChunkEl ? nel - o : amx_stage::Pool::kChunkEl});
            at += cnt;
        }
        first_chunk.push_back((int)chunks.size());
    }
    struct NarrowScope { amx_stage::Pool *p; ~NarrowScope() { if (p) p->end(); } } narrow_scope{narrow ? ctx->stage : nullptr};   // (its threads read the caller's buffer)
    if (narrow) ctx->stage->begin(reinterpret_cast<const double *>(y), chunks);
    for (int c = 0; off < n_vox; c++) {
        // the first copy is the only one the solver cannot hide: one short batch (131 072 voxels; shorter ones cost more in the
        // ~2.4 ms floor of the seeded kernel chain than their copy saves), then the rest in equal batches of <= kHostBatch voxels
        const int64_t cnt = batch_cnt(c, off);
        int b = c % kBufs;
        const double tr1 = trace ? wall() : 0.0;
        if (pipelined && c >= kBufs) {
            HIPCHK(ctx, hipEventSynchronize(ctx->hev[b]));           // batch c-3 has released this buffer
            report(done_before[b]);                                  // batches 0 .. c-3 are complete
        }
        if (two_streams) { s = (c & 1) ? ctx->hs2 : ctx->hs; if (c) ctx->swap_work(); }
        // (the uploads below are blocking hipMemcpy calls on the null stream -- from the caller's pageable memory, or from the pinned slots of the
        //  float32 transport -- and the consumers run on the non-blocking streams hs / hs2: hipMemcpy returns when the data has landed for pageable
        //  sources; for the pinned ones that is the runtime's behaviour, not its contract, so the batch's stream WAITS for an event recorded behind
        //  the batch's last copy (round 6, ADVICE r05: two API calls, ~3 us per batch))
        double *yb = ctx->hy.p ? (double *)ctx->hy.p + (size_t)b * kHostBatch * nS : nullptr;
        double *db = dirs ? (double *)ctx->hdirs.p + (size_t)b * kHostBatch * 3 : nullptr;
        const double tr2 = trace ? wall() : 0.0;
        const float *sent32 = nullptr;             // this batch's float32 signals in HBM, or null: float64 in the staging buffer
        if (kF32) {
            float *y32 = (float *)ctx->hy32.p + (size_t)b * kHostBatch * nS;
            const size_t nel = (size_t)cnt * nS;
            HIPCHK(ctx, hipMemcpy(y32, y + (size_t)off * nS, nel * sizeof(float), hipMemcpyHostToDevice));
            if (native32) sent32 = y32;
            else widen_on_device(y32, yb, nel, s);
        } else {
            bool sent = false;
            const size_t nel = (size_t)cnt * nS;
            if (narrow) {
                float *y32 = (float *)ctx->hy32.p + (size_t)b * kHostBatch * nS;
                const size_t base_el = (size_t)off * nS;
                sent = true;
                for (int j = first_chunk[c]; j < first_chunk[c + 1]; j++) {
                    // not float32 values (nothing to gain for the rest of the call either) or a failed copy: this batch and the rest go the plain way
                    if (!ctx->stage->ready(j) ||
                        hipMemcpy(y32 + (chunks[j].off - base_el), ctx->stage->slot(j), chunks[j].n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
                        (void)hipGetLastError();
                        ctx->stage->end(); narrow = false; sent = false;
                        break;
                    }
                    ctx->stage->consumed(j);
                }
                if (sent) {
                    if (native32) sent32 = y32;
                    else widen_on_device(y32, yb, nel, s);
                    ctx->host_narrowed++;
                }
            }
            if (!sent) {
                if (native32) {      // (the float64 staging buffer of a native-float32 call: needed after all -- and an earlier, smaller call's may be too small)
                    if ((rc = amx_ensure(ctx, ctx->hy, (size_t)cap * nS * sizeof(double)))) return rc;
                    yb = (double *)ctx->hy.p + (size_t)b * kHostBatch * nS;
                }
                HIPCHK(ctx, hipMemcpy(yb, y + (size_t)off * nS, (size_t)cnt * nS * sizeof(double), hipMemcpyHostToDevice));
            }
        }
        if (dirs) HIPCHK(ctx, hipMemcpy(db, dirs + (size_t)off * 3, (size_t)cnt * 3 * sizeof(double), hipMemcpyHostToDevice));
        if (ctx->up_ev) { HIPCHK(ctx, hipEventRecord(ctx->up_ev, nullptr)); HIPCHK(ctx, hipStreamWaitEvent(s, ctx->up_ev, 0)); }
        const double tr3 = trace ? wall() : 0.0;
        // the copy above took a while: has the previous batch finished meanwhile? (a query, never a wait)
        // (batches c-1 and c-2 run on different streams: both must have fired before batch c-1's count is reported)
        if (pipelined && c >= 1 && ctx->progress && hipEventQuery(ctx->hev[(c - 1) % kBufs]) == hipSuccess &&
            (c < 2 || hipEventQuery(ctx->hev[(c - 2) % kBufs]) == hipSuccess))
            report(done_before[(c - 1) % kBufs]);
        FitCall bc = call;
        bc.y = sent32 ? nullptr : yb; bc.y32 = sent32; bc.dirs = db; bc.n = cnt; bc.stream = s;
        bc.est = (double *)outs[0].buf->p + (size_t)off * outs[0].cols;
        bc.rmse = outs[1].on ? (double *)outs[1].buf->p + off : nullptr; bc.nrmse = outs[2].on ? (double *)outs[2].buf->p + off : nullptr;
        bc.extra = outs[3].on ? (double *)outs[3].buf->p + (size_t)off * outs[3].cols : nullptr;
        bc.batch = Batch{call_vox, off, true};
        if ((rc = amx_fit_dev(ctx, m, bc))) return rc;
        off += cnt;
        if (pipelined) { HIPCHK(ctx, hipEventRecord(ctx->hev[b], s)); done_before[b] = off; }
        if (trace) fprintf(stderr, "amx host trace: batch %d  %lld voxels  at %.2f ms: buffer wait %.2f, copy %.2f (%.1f GB/s), enqueue %.2f\n", c, (long long)cnt,
                           tr1 - tr0, tr2 - tr1, tr3 - tr2, ((double)cnt * nS * sizeof(T) + (dirs ? cnt * 24.0 : 0.0)) / (tr3 - tr2) * 1e-6, wall() - tr3);
    }
    ctx->profiling = call_scope.profiling;
    const double tr4 = trace ? wall() : 0.0;
    // The results of the batches that are through go home while the last ones are still being solved (the calling thread has nothing else to
    // do during the solver's tail): the voxels [0, upto) of every output are final once every batch that ends at or before `upto` has fired
    // its event -- batches older than the kBufs last ones were waited for when their staging buffer was taken again.
    int64_t copied = 0;
    auto results_upto = [&](int64_t upto) -> int {
        if (upto <= copied) return AMX_OK;
        for (HostOut &o : outs)
            if (o.on) HIPCHK(ctx, hipMemcpy((char *)o.dst + (size_t)copied * o.cols * sizeof(double), (const char *)o.buf->p + (size_t)copied * o.cols * sizeof(double),
                                            (size_t)(upto - copied) * o.cols * sizeof(double), hipMemcpyDeviceToHost));
        copied = upto;
        return AMX_OK;
    };
    const bool early_results = pipelined && !ctx->opt_host_late_results;
    if (pipelined && (ctx->progress || early_results)) {
        // the batches still in flight, in submission order: one callback as each of them completes (the queries above only
        // catch a batch that finished while the next one was being copied)
        int64_t order[kBufs]; int idx[kBufs];
        for (int b = 0; b < kBufs; b++) { order[b] = done_before[b]; idx[b] = b; }
        for (int i = 0; i < kBufs; i++) for (int j = i + 1; j < kBufs; j++) if (order[j] < order[i]) { std::swap(order[i], order[j]); std::swap(idx[i], idx[j]); }
        for (int i = 0; i < kBufs; i++) {
            if (order[i] <= 0 || order[i] >= n_vox) continue;
            HIPCHK(ctx, hipEventSynchronize(ctx->hev[idx[i]]));
            if (two_streams && i > 0 && order[i - 1] > 0) HIPCHK(ctx, hipEventSynchronize(ctx->hev[idx[i - 1]]));
            report(order[i]);
            if (early_results && (rc = results_upto(order[i]))) return rc;
        }
    }
    if (two_streams) { HIPCHK(ctx, hipStreamSynchronize(s == ctx->hs ? ctx->hs2 : ctx->hs)); }
    rc = amx_sync_status(ctx, s);
    if (rc) return rc;
    const double tr5 = trace ? wall() : 0.0;
    if ((rc = results_upto(n_vox))) return rc;
    if (trace) fprintf(stderr, "amx host trace: last enqueue at %.2f ms, solver tail %.2f, results to the host %.2f, call %.2f ms, %d batches as float32\n", tr4 - tr0, tr5 - tr4, wall() - tr5, wall() - tr0, ctx->host_narrowed);
    progress(ctx, n_vox, n_vox);
    return AMX_OK;
}

// the checks of a host-buffer call (their messages are not the device entry points'), its outputs, the call
template <typename T>
int fit_any(amx_ctx *ctx, const FitSpec &m, const T *y, const FitCall &c)
{
    if (!ctx) return AMX_E_BADARG;
    if (!c.lut || c.lut->model != m.model) return fit_bad(ctx, m, ": not a ", " dictionary");
    if (c.n == 0) return AMX_OK;
    if (c.n < 0 || !y || (m.dirs && !c.dirs) || !c.est) return fit_bad(ctx, m, ": bad argument");
    if (((c.flags & AMX_F_RMSE) && !c.rmse) || ((c.flags & AMX_F_NRMSE) && !c.nrmse) || ((c.flags & m.extra_flag) && !c.extra)) return fit_bad(ctx, m, ": flag set but output buffer is null");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HostOut outs[4] = {{c.est, &ctx->hest, (size_t)fit_maps(m, c), true},
                       {c.rmse, &ctx->hrmse, 1, (c.flags & AMX_F_RMSE) != 0}, {c.nrmse, &ctx->hnrmse, 1, (c.flags & AMX_F_NRMSE) != 0},
                       {c.extra, &ctx->hextra, (size_t)(m.extra_cols ? m.extra_cols : c.lut->nS), (c.flags & m.extra_flag) != 0}};
    // (every NODDI kernel reads float32 signals in place -- the table GEMM, the wavefront-per-voxel kernels' load_rows, the rescue pass --: a batch
    //  that crossed the link as float32 is fitted as float32, no widened copy; bit-identical maps: amx_noddi_fit_device_f32)
    return fit_host<T>(ctx, m, c, y, m.model == 1, outs);
}

}  // namespace

// Round 6: the pool is made WHILE the dictionary is uploaded.  Pinning its 64 MB ring and starting its threads takes ~15 ms, and it used to
// happen inside the first host-buffer fit of a process -- the one fit a subject gets (core.py:465-466: one model.fit per Evaluation) --
// behind 10 ms of dictionary tables built on the GPU and a digest of KERNELS on the host: a helper thread makes the pool beside those, the
// first fit adopts it (NODDI().fit(evaluation), first call of a process, 1 M voxels: 41.6 ms -> see profiles/r06_first_call.txt).
void prefetch_stage_pool(amx_ctx *ctx)
{
    if (ctx->stage || ctx->stage_failed || ctx->stage_bg_started || ctx->opt_host_no_narrow) return;
    if (ctx->opt_host_pin == 'c' || ctx->opt_host_no_prefetch) return;          // (the caller's node is the CALLING thread's: made where it is needed)
    ctx->stage_bg_started = true;
    try {
        ctx->stage_thread = std::thread([ctx] {
            if (hipSetDevice(ctx->device) != hipSuccess) { (void)hipGetLastError(); return; }
            ctx->stage_bg = make_stage_pool(ctx);
        });
    } catch (...) { ctx->stage_bg_started = false; }
}

extern "C" {

int amx_noddi_fit(amx_ctx *ctx, const amx_lut *lut, const double *y, const double *dirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *out_estimates, double *out_rmse, double *out_nrmse, double *out_mod)
{
    return fit_any(ctx, kFits[0], y, {lut, nullptr, nullptr, dirs, n_vox, lambda1, lambda2, 0, flags, out_estimates, out_rmse, out_nrmse, out_mod, nullptr, {}});
}
int amx_noddi_fit_f32(amx_ctx *ctx, const amx_lut *lut, const float *y, const double *dirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *out_estimates, double *out_rmse, double *out_nrmse, double *out_mod)
{
    return fit_any(ctx, kFits[0], y, {lut, nullptr, nullptr, dirs, n_vox, lambda1, lambda2, 0, flags, out_estimates, out_rmse, out_nrmse, out_mod, nullptr, {}});
}

int amx_freewater_fit(amx_ctx *ctx, const amx_lut *lut, const double *y, const double *dirs, int64_t n_vox, double lambda1, double lambda2, int is_mouse, unsigned flags, double *out_estimates, double *out_rmse, double *out_nrmse, double *out_ycorr)
{
    return fit_any(ctx, kFits[1], y, {lut, nullptr, nullptr, dirs, n_vox, lambda1, lambda2, is_mouse, flags, out_estimates, out_rmse, out_nrmse, out_ycorr, nullptr, {}});
}
int amx_freewater_fit_f32(amx_ctx *ctx, const amx_lut *lut, const float *y, const double *dirs, int64_t n_vox, double lambda1, double lambda2, int is_mouse, unsigned flags, double *out_estimates, double *out_rmse, double *out_nrmse, double *out_ycorr)
{
    return fit_any(ctx, kFits[1], y, {lut, nullptr, nullptr, dirs, n_vox, lambda1, lambda2, is_mouse, flags, out_estimates, out_rmse, out_nrmse, out_ycorr, nullptr, {}});
}

int amx_sandi_fit(amx_ctx *ctx, const amx_lut *lut, const double *y, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *out_estimates, double *out_rmse, double *out_nrmse)
{
    return fit_any(ctx, kFits[2], y, {lut, nullptr, nullptr, nullptr, n_vox, lambda1, lambda2, 0, flags, out_estimates, out_rmse, out_nrmse, nullptr, nullptr, {}});
}
int amx_sandi_fit_f32(amx_ctx *ctx, const amx_lut *lut, const float *y, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *out_estimates, double *out_rmse, double *out_nrmse)
{
    return fit_any(ctx, kFits[2], y, {lut, nullptr, nullptr, nullptr, n_vox, lambda1, lambda2, 0, flags, out_estimates, out_rmse, out_nrmse, nullptr, nullptr, {}});
}

int amx_czb_fit(amx_ctx *ctx, const amx_lut *lut, const double *y, const double *dirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *out_estimates, double *out_rmse, double *out_nrmse)
{
    return fit_any(ctx, kFits[3], y, {lut, nullptr, nullptr, dirs, n_vox, lambda1, lambda2, 0, flags, out_estimates, out_rmse, out_nrmse, nullptr, nullptr, {}});
}
int amx_czb_fit_f32(amx_ctx *ctx, const amx_lut *lut, const float *y, const double *dirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *out_estimates, double *out_rmse, double *out_nrmse)
{
    return fit_any(ctx, kFits[3], y, {lut, nullptr, nullptr, dirs, n_vox, lambda1, lambda2, 0, flags, out_estimates, out_rmse, out_nrmse, nullptr, nullptr, {}});
}

}  // extern "C"
