// amx_host.hpp -- host-side context shared by the entry-point units (amx_api / amx_plan / amx_lut / amx_fit_dev / amx_fit_host) and the per-model launch units.
#pragma once
#include "../../include/amico_amd.h"
#include "amx_kernels.hpp"
#include "amx_noddi_route.hpp"
#include "amx_small_route.hpp"
#include "amx_stage.hpp"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

constexpr int kListGrid = 512;     // workgroups of the large-MAXP re-run pass
constexpr int kEv = 20;           // event pairs: 0 whole call, 1-3 NODDI stage kernels, 4 small-model solver, 5-7 NODDI GEMM + seed + certificate kernels of stages 1 / 2 / 3, 8 k_nnls_seed<1> alone, 9 k_lasso_seed alone

struct DevBuf {
    void *p = nullptr; size_t cap = 0;
};

// The per-call workspace (stream-ordered, grow-only): ONE list.  A buffer added here is swapped between the two streams of a host-buffer call
// and freed with the context; nothing else names the members.
#define AMX_WORK_BUFS(X) X(lutidx) X(perm) X(counts) X(dir_start) X(cursor) X(chunks) X(misc) X(xiso) X(supp) X(ovf) X(cproj) X(ytil) X(seeds) \
    X(schunks) X(ytil2) X(seeds2) X(cgemm) X(done) X(rlist) X(cgemm2) X(clip) X(feed)
struct WorkSet {
#define X(name) DevBuf name;
    AMX_WORK_BUFS(X)
#undef X
    template <typename F> void for_each(F f) {
#define X(name) f(name);
        AMX_WORK_BUFS(X)
#undef X
    }
};

// Where a device fit stands in the call it belongs to: a device-pointer call is its own call (the default); fit_host enqueues the batches of a
// host-buffer call with theirs.  Batches of one call all take the paths the WHOLE call's size asks for (bit-identical to the one-shot call).
struct Batch {
    int64_t call_vox = 0;          // voxels of the whole call (0: this fit's own)
    int64_t base = 0;              // index of this batch's first voxel in the call
    bool host = false;             // inside a host-buffer call: it reports progress per batch itself
    bool first() const { return base == 0; }
};

struct amx_ctx : WorkSet {
    int device = 0;
    int n_cu = 256;                // compute units of the device (persistent-grid launches)
    std::string err;
    WorkSet alt;                   // second workspace set for the batch in flight on the other stream
    void swap_work() { std::swap(static_cast<WorkSet &>(*this), alt); work_idx ^= 1; }
    DevBuf big;                    // factor blocks of k_noddi_lasso_big for dictionaries of more than 176 candidate atoms (amx_big.hip)
    DevBuf hy, hdirs, hest, hrmse, hnrmse, hextra;   // staging for the host-pointer entry points
    int *status_d = nullptr;       // ST_WORDS ints
    int *status_h = nullptr;       // pinned mirror (+16 words: copy of the misc counters)
    int profiling = 0;             // 0 off, 1 every event pair of a call, 2 + w: pair w only (amx_set_profiling)
    int64_t call_vox = 0;          // voxels of the call being enqueued (the whole host-buffer call for its batches): every size-dependent path choice reads this
    Batch batch;                   // of the fit being enqueued (fit_check sets both; fit_host clears it when the call is over)
    int64_t call_total_vox = 0;    // amx_set_call_voxels: the host-buffer calls on this ctx are shards of a call of this many voxels (0: they are the call)
    hipEvent_t ev[kEv];
    bool ev_valid[kEv];
    int64_t stats[4] = {0, 0, 0, 0};
    int64_t seed_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // amx_last_seed_stats
    int64_t dense_stats[2] = {0, 0};   // amx_batched_last_dense: voxels k_batched_big solved in the last synchronised call, its pivoting steps
    int64_t uncert_vox[3] = {0, 0, 0};   // ... of which a stage ran without its Gram-space certificate (shape gate, AMX_NO_GCERT)
    int64_t seeded_vox = 0;        // voxels enqueued on the seed -> certificate chain since the last amx_sync_status
    double *dbg_x = nullptr;       // AMX_F_DEBUG_X destination (caller-owned device buffer, amx_set_debug_x)
    double *fw_iso = nullptr;      // AMX_F_FW_ISO destination (caller-owned device buffer, amx_set_fw_iso)
    void (*progress)(int64_t, int64_t, void *) = nullptr;   // amx_set_progress
    void *progress_user = nullptr;
    DevBuf wy;                     // float64 copy of float32 device signals for the lane kernels that read float64 only (amx_*_fit_device_f32)
    DevBuf pred_idx;               // LUT index of every row of the last amx_predict_device / amx_prep_predicted_device call (amx_predict.hip)
    DevBuf hy32;                   // float32 signals of the *_fit_f32 entry points (and of float64 host signals that are float32 values: amx_stage.hpp)
    amx_stage::Pool *stage = nullptr;  // host threads + pinned slots of the lossless float64 -> float32 transport (made at the first large float64 host call)
    std::thread stage_thread;      // makes the pool beside the dictionary upload (prefetch_stage_pool); joined by the first host-buffer fit that needs it
    amx_stage::Pool *stage_bg = nullptr;
    bool stage_bg_started = false;
    bool stage_failed = false;     // the pool could not be made: host signals are copied as they are
    int host_narrowed = 0;         // batches of the last host-buffer call that travelled as float32 (amx_last_host_narrowed)
    hipStream_t hs = nullptr;      // non-blocking compute streams of the chunked host entry points: batches alternate
    hipStream_t hs2 = nullptr;     // between the two, so the tail of one batch's kernels is filled by the next batch's
    hipEvent_t hev[3] = {nullptr, nullptr, nullptr};
    hipEvent_t up_ev = nullptr;    // recorded on the null stream behind a batch's uploads; the batch's compute stream waits for it
    // environment switches: read ONCE, by amx_ctx_create on the caller's thread, through kSwitches below -- the table is their documentation
    bool opt_no_seed, opt_no_gcert, opt_no_gcert_wide, opt_no_screen, opt_s2_exact, opt_no_chunk_order, opt_no_hard_first, opt_no_big_all;
    bool opt_wave_per_voxel, opt_no_refill, opt_sandi_atom_space, opt_fw_no_fuse, opt_prep_scalar, opt_debug;
    bool opt_host_one_shot, opt_host_late_results, opt_host_no_native32, opt_host_no_narrow, opt_host_no_prefetch, opt_host_trace;
    long long opt_seed_stages, opt_seed_chunk, opt_seed_waves, opt_seed_min_voxels, opt_seed_occ2_from, opt_seed2_occ2_from, opt_seed_tripcap[3];
    long long opt_rescue_from, opt_gcert_repair, opt_gcert2_third, opt_fork;
    long long opt_host_threads, opt_host_batch, opt_host_ramp, opt_host_pipeline_from, opt_host_pin, opt_host_pin_cores, opt_host_siblings[3];
    long long opt_local_rank, opt_local_world;
    hipStream_t fork_s[2] = {nullptr, nullptr};          // (one per workspace set: work_idx)
    hipEvent_t fork_ev[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
    int work_idx = 0;               // which of the two workspace sets the named buffers are (swap_work)
    bool side_launch = false;       // transient: the launch being enqueued goes to the side stream (launch_pair picks its own overflow lists)
    std::string path;               // kernels of the last fit enqueued on this ctx, in launch order (amx_last_path)
    // Rician debias (amx_debias.hip): sigma of every voxel / row of the call in flight, its b0 list, and the counter of samples that
    // reached the trip cap in the last call (amx_debias_last_unconverged), read behind the event recorded after that call's kernels
    DevBuf debias_sigma, debias_b0;
    unsigned long long *debias_stats = nullptr;
    hipEvent_t debias_ev = nullptr;
    // NaN / Inf scan (amx_sanitize.hip): counters of the last two calls, alternating, each read behind the event recorded after its kernel
    unsigned long long *san_count = nullptr;
    unsigned long long *san_host = nullptr;    // pinned mirror of the two counters, written by a copy enqueued behind each scan
    hipEvent_t san_ev[2] = {nullptr, nullptr};
    unsigned san_seq = 0;          // sanitize calls enqueued on this ctx so far; call k counts into san_count[k & 1]
    // exact median (amx_noise.hip): a ring of slots (state + one histogram pair per digit pass); call k takes slot k mod kMedRing
    DevBuf median_ws;
    unsigned median_seq = 0;
    // Gibbs unringing (amx_unring.hip): the tables and one chunk of slices in float64, never more than amx::kUnringScratchCap bytes
    DevBuf unring_ws;
};

// ------------------------------------------------------------------ environment switches
// One row per switch: name, kind, the amx_ctx field it fills, default, the rule a given number goes through, and its description (the only
// documentation of the field; DESIGN.md, "Switches", lists the same rows).  amx_ctx_create walks the table on the caller's thread; nothing else
// in the library reads the environment.  All are diagnosis / A-B tools but the AMX_HOST_* placement and batch-plan set: the defaults are the product path.
enum amx_sw_kind {
    SW_FLAG,   // on when set to anything but "" and "0..."
    SW_OFF,    // "=0 disables": the field (opt_no_* / opt_*_no_*) is true when the value starts with '0'
    SW_GIVEN,  // on when the variable exists, whatever its value
    SW_CHAR,   // the value's first character (the default when the variable does not exist)
    SW_INT,    // an integer; `fix` clamps / rounds it, or returns the default to ignore it ("" is ignored)
    SW_LIST    // up to three integers in `fmt`; the ones not given keep their defaults, every one goes through `fix`
};
struct amx_switch {
    const char *name; amx_sw_kind kind;
    bool amx_ctx::*flag; long long amx_ctx::*num; long long (amx_ctx::*list)[3];
    long long dflt[3];
    long long (*fix)(long long v, long long dflt);
    const char *fmt, *doc;
};
constexpr long long sw_any(long long v, long long) { return v; }
constexpr long long sw_not_negative(long long v, long long) { return v < 0 ? 0 : v; }
constexpr long long sw_zero_one(long long v, long long) { return v != 0 ? 1 : 0; }
constexpr amx_switch sw_flag(const char *n, bool amx_ctx::*f, const char *doc) { return {n, SW_FLAG, f, nullptr, nullptr, {0, 0, 0}, nullptr, nullptr, doc}; }
constexpr amx_switch sw_off(const char *n, bool amx_ctx::*f, const char *doc) { return {n, SW_OFF, f, nullptr, nullptr, {0, 0, 0}, nullptr, nullptr, doc}; }
constexpr amx_switch sw_given(const char *n, bool amx_ctx::*f, const char *doc) { return {n, SW_GIVEN, f, nullptr, nullptr, {0, 0, 0}, nullptr, nullptr, doc}; }
constexpr amx_switch sw_char(const char *n, long long amx_ctx::*f, long long d, const char *doc) { return {n, SW_CHAR, nullptr, f, nullptr, {d, 0, 0}, nullptr, nullptr, doc}; }
constexpr amx_switch sw_int(const char *n, long long amx_ctx::*f, long long d, long long (*fix)(long long, long long), const char *doc) { return {n, SW_INT, nullptr, f, nullptr, {d, 0, 0}, fix, nullptr, doc}; }
constexpr amx_switch sw_list(const char *n, long long (amx_ctx::*f)[3], long long d0, long long d1, long long d2, long long (*fix)(long long, long long), const char *fmt, const char *doc) { return {n, SW_LIST, nullptr, nullptr, f, {d0, d1, d2}, fix, fmt, doc}; }

inline constexpr amx_switch kSwitches[] = {
    // ---- NODDI: which kernels a fit takes
    sw_flag("AMX_NO_SEED", &amx_ctx::opt_no_seed, "Lawson-Hanson from the empty set in the NNLS stages (the round-2 path)"),
    sw_flag("AMX_NO_GCERT", &amx_ctx::opt_no_gcert, "every seed is certified by the wavefront-per-voxel kernels (true residual)"),
    sw_flag("AMX_NO_GCERT_WIDE", &amx_ctx::opt_no_gcert_wide, "no second Gram-certificate pass for LASSO supports of 12 .. 18 atoms"),
    sw_flag("AMX_NO_SCREEN", &amx_ctx::opt_no_screen, "certify seeds with the full exact sweep of the dual vector"),
    sw_flag("AMX_S2_EXACT", &amx_ctx::opt_s2_exact, "every voxel's stage-2 products by the exact pass (k_noddi_gemm<true>), none derived from the stage-1 table"),
    sw_int("AMX_SEED_STAGES", &amx_ctx::opt_seed_stages, 7, [](long long v, long long) { return v & 7; }, "bit 0 = seed stage 1, bit 1 = seed stage 3, bit 2 = seed the LASSO stage"),
    // (never below kChunk: the left-over passes size their grid by the FIRST plan's chunk count, n / kChunk + ndirs + 1.  Lanes refill from the
    //  chunk: the more voxels per lane, the smaller the share of the tail; 1 M voxels: 1024 -> 7.2 ms, 2048 -> 7.3, 4096 -> 5.5 for stage 1)
    sw_int("AMX_SEED_CHUNK", &amx_ctx::opt_seed_chunk, 0, [](long long v, long long d) { return v >= kChunk ? ((v + 63) & ~63LL) : d; },
           "voxels of one orientation per workgroup of the seed solvers (at least 256, rounded up to a multiple of 64; 0 = by the call's size, noddi_route)"),
    sw_int("AMX_SEED_WAVES", &amx_ctx::opt_seed_waves, 0, [](long long v, long long) { return (v == 1 || v == 2 || v == 4) ? v : 0; },
           "wavefronts per workgroup of the lane kernels: 1, 2 or 4 (0 = by the number of chunks, noddi_route)"),
    // (the seeded chain of ~16 kernels has a floor of ~1.5 ms; measured, tools/r04/round8.sh: 20 000 voxels 1.58 against 1.49 ms, 25 000 voxels 1.60 against 1.78, 40 000 1.70 against 2.34)
    sw_int("AMX_SEED_MIN_VOXELS", &amx_ctx::opt_seed_min_voxels, 22528, sw_any, "smaller calls run the wavefront-per-voxel kernels on all voxels"),
    // (a third more time per trip, twice the wavefronts: wins when the kernel is throughput bound -- 1 M voxels 2.80 -> 2.14 ms --, loses when the longest voxel's path bounds it:
    //  50 000 voxels 0.54 -> 0.73 ms; with four wavefronts per workgroup the crossover sits between 200 000 and 300 000 voxels; k_lasso_seed: 200 000 voxels 0.50 -> 0.42 ms, 1 M: 1.67 -> 1.27 ms)
    sw_int("AMX_SEED_OCC2_FROM", &amx_ctx::opt_seed_occ2_from, 65536, sw_any, "calls of at least this many voxels run k_nnls_seed<1> at two wavefronts per SIMD"),
    sw_int("AMX_SEED2_OCC2_FROM", &amx_ctx::opt_seed2_occ2_from, 65536, sw_any, "the same for k_lasso_seed"),
    // A lane kernel lasts as long as its slowest voxel, and the slowest are a handful: of 1 M bench voxels 12 need more than 32 stage-1 trips (mean ~10), yet
    // with the old cap of 64 they held the kernel 0.4 ms longer.  Measured (tools/r04/tripcap2.sh; 50 000 / 200 000 / 1 M voxels, fit in ms): 64,64,64 2.09 /
    // 3.31 / 8.17; 28,24,12 1.74 / 2.94 / 7.66; below 20 / 18 / 8 the left-over kernels get more voxels than the shorter tails are worth.  (28, 24, 12 before
    // the normalised entering rule shortened the paths, 24, 24, 10 until the stage-1 solver handed its support on and the LASSO left-over solver started
    // from the seed: profiles/r05b_tripcaps.txt)
    sw_list("AMX_SEED_TRIPCAP", &amx_ctx::opt_seed_tripcap, 20, 20, 10, [](long long v, long long) { return v < 4 ? 4 : v; }, "%lld,%lld,%lld",
            "a,b,c: trips after which k_nnls_seed<1> / k_lasso_seed / k_nnls_seed<3> give a voxel up (at least 4; no seed: it goes to the left-over kernels)"),
    sw_flag("AMX_NO_CHUNK_ORDER", &amx_ctx::opt_no_chunk_order, "the chunks of the second plan stay in orientation order (default: longest first)"),
    sw_flag("AMX_NO_HARD_FIRST", &amx_ctx::opt_no_hard_first, "the left-over kernels of the NNLS stages walk their lists in the order the certificates wrote them"),
    sw_int("AMX_RESCUE_FROM", &amx_ctx::opt_rescue_from, -1, sw_not_negative,
           "calls of n voxels and more run the rescue pass of the NNLS certificates (k_nnls_gcert<., true>), and the threshold alone decides (not given: kRescueFrom, and every call of a protocol of more than 128 volumes)"),
    sw_int("AMX_GCERT_REPAIR", &amx_ctx::opt_gcert_repair, -1, sw_zero_one, "0 / 1: never / always the NNLS certificates' second look at a mendable seed (default: where the tile is read from L2)"),
    sw_int("AMX_GCERT2_THIRD", &amx_ctx::opt_gcert2_third, -1, sw_zero_one, "0 / 1: never / always a third LASSO certificate pass (default: where the tile is read from L2, and large calls of 96 .. 128 volumes)"),
    sw_off("AMX_BIG_ALL", &amx_ctx::opt_no_big_all, "=0: lambda1 = 0 fits take the fast kernels first and reach k_noddi_lasso_big through the overflow lists"),
    // (round 6: a recorded negative result, profiles/r06_fork_negative.txt.  Bit 1 is a correct fit -- the forked voxels skip the stage-3 lane kernels and end in
    //  k_noddi<3> on the side stream; bit 0 is a TIMING PROBE only: the stage-2 lane kernels read the x_iso the previous call left for those voxels)
    sw_int("AMX_FORK", &amx_ctx::opt_fork, 0, [](long long v, long long) { return v & 3; },
           "bit 0 / bit 1: the left-over kernels of stage 1 / of the LASSO stage run on a side stream beside the next stage's lane kernels (noddi_fit_dev)"),
    // ---- the small models, signal preparation
    sw_flag("AMX_WAVE_PER_VOXEL", &amx_ctx::opt_wave_per_voxel, "small models by the wavefront-per-voxel kernels"),
    sw_flag("AMX_NO_REFILL", &amx_ctx::opt_no_refill, "FreeWater by k_freewater_lane (one solve per lane and pass)"),
    sw_flag("AMX_FW_NO_FUSE", &amx_ctx::opt_fw_no_fuse, "FreeWater by the projection + solver kernel pair instead of k_freewater_fused"),
    sw_flag("AMX_SANDI_ATOM_SPACE", &amx_ctx::opt_sandi_atom_space, "SANDI 6 x 15 by the atom-space lane kernel"),
    sw_flag("AMX_PREP_SCALAR", &amx_ctx::opt_prep_scalar, "the streaming preparation kernel with one voxel per lane (4-byte loads) instead of four (tools/r04/prep.sh)"),
    // ---- the host-buffer entry points (README.md, "Behaviour-changing defaults of the host-buffer calls")
    sw_flag("AMX_HOST_ONE_SHOT", &amx_ctx::opt_host_one_shot, "host-buffer entry points upload everything, then fit"),
    sw_flag("AMX_HOST_LATE_RESULTS", &amx_ctx::opt_host_late_results, "the results of a host-buffer call go home in one copy after the last batch"),
    sw_off("AMX_HOST_NATIVE32", &amx_ctx::opt_host_no_native32, "=0: float32 batches are widened on the device first (the round-5 behaviour)"),
    sw_off("AMX_HOST_NARROW", &amx_ctx::opt_host_no_narrow, "=0: float64 host signals are always copied as they are (amx_stage.hpp)"),
    // (from 3 x 131 072 voxels a call has two batches -- the first short -- and the second copy hides behind the first fit: 400 000 voxels 7.63 -> 6.85 ms (float32 signals 6.94 -> 6.08),
    //  500 000 8.66 -> 7.92 (8.30 -> 7.51); was 524 288 while a float64 copy took twice as long (profiles/r05c_host_transport.txt, section 9))
    sw_int("AMX_HOST_PIPELINE_FROM", &amx_ctx::opt_host_pipeline_from, 393217, [](long long v, long long d) { return v >= 262144 ? v : d; },
           "host-buffer calls of fewer voxels upload everything, then fit (at least 262144: a pipelined call has a first batch of 131 072 voxels and a second one at least as long)"),
    sw_int("AMX_HOST_RAMP", &amx_ctx::opt_host_ramp, 131072, [](long long v, long long) { return v <= 0 ? 0 : (v > 131072 ? 131072 : ((v + 3) & ~3LL)); },
           "voxels of the first pipelined batch (its copy is the only one nothing hides; at most 131072, a multiple of 4; 0 = equal batches)"),
    sw_int("AMX_HOST_BATCH", &amx_ctx::opt_host_batch, 393216, [](long long v, long long d) { return v >= 131072 ? ((v + 3) & ~3LL) : d; },
           "voxels per pipelined batch (a multiple of 4: k_widen reads float4; at least the largest ramp batch, 131072: the ramp batches are written into slots of this size)"),
    sw_int("AMX_HOST_THREADS", &amx_ctx::opt_host_threads, 12, [](long long v, long long d) { return v >= 1 ? (v > 64 ? 64 : v) : d; },
           "host threads that narrow + send float64 host signals (1 .. 64; at most half the logical CPUs)"),
    sw_char("AMX_HOST_PIN", &amx_ctx::opt_host_pin, 'g', "gpu / caller / 0: those threads run on the device's NUMA node (their share of its cores), on the calling thread's node, anywhere"),
    sw_char("AMX_HOST_PIN_CORES", &amx_ctx::opt_host_pin_cores, 0, "0: the threads share the node's CPUs as one set, 1: one core per thread (default: a stripe of the node's physical cores each)"),
    sw_off("AMX_HOST_PREFETCH", &amx_ctx::opt_host_no_prefetch, "=0: the pool of those threads is made inside the first fit that needs it instead of beside the dictionary upload"),
    sw_list("AMX_HOST_SIBLINGS", &amx_ctx::opt_host_siblings, -1, 0, 0, sw_any, "%lld/%lld", "i/n: the pool takes the i-th of n shares of its node's cores, whatever devices hang on the node (diagnosis, tests)"),
    // (set by the launcher, one visible device per process: who else drives a device of this node -- amx_stage::device_siblings)
    sw_int("LOCAL_RANK", &amx_ctx::opt_local_rank, -1, sw_any, "the launcher's (torchrun) local rank: with LOCAL_WORLD_SIZE, this process's share of the node's cores"),
    sw_int("LOCAL_WORLD_SIZE", &amx_ctx::opt_local_world, -1, sw_any, "the launcher's number of processes on this host"),
    // ---- tracing
    sw_given("AMX_HOST_TRACE", &amx_ctx::opt_host_trace, "wall-clock timeline of every host-buffer call on stderr: per batch the wait for its buffer, its copy, its enqueue (tools/r05/host_trace.py)"),
    sw_flag("AMX_DEBUG", &amx_ctx::opt_debug, "synchronise after every launch and trace progress and counters on stderr"),
};

// (defaults of switches that were retired with nothing setting them -- kLeftSmall1, kLeftSmall3 -- and kRescueFrom: amx_noddi_route.hpp, with their measurements)
// the switches that steer a NODDI fit's route, as noddi_route() takes them
inline amx::NoddiSwitches noddi_switches(const amx_ctx *c)
{
    return {c->opt_no_seed, c->opt_no_gcert, c->opt_no_gcert_wide, c->opt_no_screen, c->opt_no_big_all, c->opt_seed_stages, c->opt_seed_chunk, c->opt_seed_waves,
            c->opt_seed_min_voxels, c->opt_seed_occ2_from, c->opt_seed2_occ2_from, c->opt_rescue_from, c->opt_gcert_repair, c->opt_gcert2_third, c->opt_fork};
}

constexpr int kDictModel = 100;   // amx_dict::model

struct amx_lut {
    amx_ctx *ctx = nullptr;
    int model = 0;                 // 1 NODDI, 2 FreeWater, 3 SANDI, 4 CylinderZeppelinBall
    int nS = 0, ldA = 0, n_atoms = 0, ndirs = 0, tile_stride = 0;
    int n_wm = 0, is_exvivo = 0;   // NODDI
    int n_dwi = 0;                 // NODDI: rows of the stage-2 problem (scheme.dwi_idx; the single-b0 rule may add one)
    int n_perp = 0, n_iso = 0;     // FreeWater
    int n_rs = 0, n_in = 0, n_isos = 0;   // SANDI
    void *tiles = nullptr;
    double *gram = nullptr, *gram_dwi = nullptr;   // per-orientation Gram matrices (NODDI; gram: CylinderZeppelinBall, and every dictionary of more than 64 atoms)
    double *basis_U = nullptr, *basis_S = nullptr; // per-orientation compressed basis and dictionary (amx_seed.hpp), NODDI
    double *screen2_kappa0 = nullptr;
    double *u2iso = nullptr;       // [ndirs][12] U2'iso (amx_build_basis)
    int s2_derive = 0;             // b0 rows of every atom are exactly 1.0 and iso > 0 on the stage-2 rows: stage-2 products derive from the stage-1 table
    float *screen2_S = nullptr; double *screen2_kappa = nullptr; // the same for the LASSO stage's dictionary
    double *screen_kappa0 = nullptr;                             // max ||(I - U U') a_j|| per orientation (k_nnls_gcert)
    float *screen_S = nullptr; double *screen_kappa = nullptr;   // float32 S [ndirs][12][192] + kappa [ndirs]: dual-value screening
    double *basis2_U = nullptr, *basis2_S = nullptr;   // the same for the LASSO stage's dictionary (DWI rows, normalised atoms)
    int ldG = 0;
    short *htable = nullptr;
    unsigned char *rowdwi = nullptr;
    double *colscale = nullptr;
    float *icvf = nullptr, *kappa = nullptr;
    double *norms = nullptr, *Rs = nullptr, *d_in = nullptr, *d_isos = nullptr;
    // FreeWater, per orientation and for one lambda2 (k_fw_orient_prep, rebuilt when lambda2 changes): fp64 dictionary
    // A [nS][NP], H^-1 [N][NP], H = A'A + lambda2 I [N][N]
    mutable double *fw_prep = nullptr;
    mutable double fw_lam2 = -1.0;
    mutable int fw_N = 0;
    mutable hipEvent_t fw_ready = nullptr;
    // CylinderZeppelinBall fast path (amx_czb.hip), per orientation and for one lambda2: M = (A'A + lambda2 I)^-1, M 1, M A'
    mutable double *czb_prep = nullptr;
    mutable double czb_lam2 = -1.0;
    mutable hipEvent_t czb_ready = nullptr;
    // SANDI row-space solver tables (k_sandi_tables) for one (lambda1, lambda2)
    mutable double *sandi_prep = nullptr;
    mutable double sandi_lam1 = -1.0, sandi_lam2 = -1.0;
    mutable hipEvent_t sandi_ready = nullptr;
    // SANDI on protocols of more than 128 volumes (amx_sandi_long.hip), for one lambda2: G = A'A, H = G + lambda2 I, A' in MFMA operand order
    mutable double *sandi_long_prep = nullptr;
    mutable double sandi_long_lam2 = -1.0;
    mutable hipEvent_t sandi_long_ready = nullptr;
};

// dictionaries of the batched solver entry points (amx_nnls_batched / amx_lasso_batched)
struct amx_dict {
    amx_ctx *ctx = nullptr;
    int model = kDictModel;        // where amx_lut holds its model: amx_debug_fetch tells the two kinds of handle apart by it
    int m = 0, n = 0, ldA = 0, tile_stride = 0, n_dicts = 0;
    double *tiles = nullptr;       // device f64 [n_dicts][m][ldA] (row-major, odd leading dimension)
    // amx_dict_set_dense: the Gram matrices G_d = A_d'A_d, device f64 [n_dicts][n][ldG]; voxels whose support outgrows the 48-atom re-run
    // pass go to k_batched_big (amx_batched_big.hip) instead of AMX_E_OVERFLOW
    bool dense = false;
    double *gram = nullptr;
    int ldG = 0;
};

// principal-direction estimator of one acquisition scheme (amx_signal.hip)
struct amx_dti {
    amx_ctx *ctx = nullptr;
    int nS = 0;
    double min_signal = 0.0;
    double *wt = nullptr;          // device f64[nS][6]: transposed first six rows of pinv(design matrix)
    int method = 0;                // AMX_DTI_OLS | AMX_DTI_WLS | AMX_DTI_NLLS | AMX_DTI_RESTORE
    double sigma = 0.0;            // RESTORE: the noise level
    // all but OLS (one allocation): pinv(design)^T and the design matrix, f64[nS][7] each, in the column-scaled
    // parametrisation; 1 / scale; counters of the last NLLS / RESTORE call, kDtiStats of them (unconverged voxels, voxel trips,
    // wavefront trips, -, RESTORE: voxels in step 3, refitted, at step 3's cap, with fewer than 7 inliers)
    double *wt7 = nullptr, *xs = nullptr;
    double ics[7] = {1, 1, 1, 1, 1, 1, 1};
    unsigned long long *stats = nullptr;
    mutable hipStream_t last_stream = nullptr;
};

// signal preparation plan of one (image geometry, mask, scheme, options) combination (amx_volume.hip)
struct amx_prep {
    amx_ctx *ctx = nullptr;
    long long d[3] = {0, 0, 0};    // spatial extents, d[0] = axis that is fastest in the image's memory
    long long s[3] = {0, 0, 0};    // element strides of those axes in the image
    long long c[3] = {0, 0, 0};    // strides of those axes in a C-ordered [X][Y][Z] volume
    long long sv = 0;              // element stride of the volume axis
    int ax[3] = {0, 1, 2};         // the caller's axis (0, 1, 2 of dims) that d[k] / s[k] / c[k] speak of
    long long extent = 0;          // elements spanned by the image (largest offset + 1)
    long long n_total = 0, n_vox = 0;
    int nS = 0, n_out = 0, n_b0 = 0, n_gidx = 0, identity = 0, inplace = 0, hazard = 0, layout = 0;   // layout: 1 planar (s[0]==1), 2 interleaved (sv==1), 0 generic
    int *rank = nullptr;           // device int32[d2][d1][d0]: index in the masked list or -1
    long long *cidx = nullptr;     // device int64[n_vox]: C-order linear index of the masked voxels
    int *gptr = nullptr, *gidx = nullptr, *b0idx = nullptr;
    // tiles of 64 voxels along the fastest axis that hold at least one masked voxel, made once with the plan: the wavefronts of
    // k_prep_gather draw from this list through a counter of `tile_counter` (a ring: launch k of the plan zeroes and uses entry
    // k mod kCounterRing on its own stream, so up to kCounterRing gathers of one plan may be in flight together): an
    // image is half background, and a strided walk over ALL tiles left some wavefronts with seven full tiles and others with none
    static constexpr int kCounterRing = 16;
    int *live64 = nullptr, *tile_counter = nullptr;
    unsigned char *dmask = nullptr; // device u8[d2][d1][d0]: mask != 0 (amx_prep_set_debias_mask; null until then)
    mutable unsigned launch_seq = 0;
    long long n_live64 = 0;
    // what the plan's last gather launched (amx_prep_last_launch): kernel name, workgroups, threads per workgroup, LDS bytes
    mutable const char *last_kernel = "";
    mutable long long last_launch[3] = {0, 0, 0};
};

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            char b_[512];                                                                         \
            snprintf(b_, sizeof b_, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, \
                     __LINE__, #call);                                                            \
            (ctx)->err = b_;                                                                      \
            return AMX_E_HIP;                                                                     \
        }                                                                                         \
    } while (0)

// amx_last_path: every launch site names its kernel (the first batch of a host-buffer call only)
static inline void amx_note(amx_ctx *ctx, const char *kernel)
{
    if (!ctx->batch.first() || ctx->path.size() > 1500) return;
    if (!ctx->path.empty()) ctx->path += " -> ";
    ctx->path += kernel;
}

static inline int amx_bad(amx_ctx *ctx, const char *msg)
{
    if (ctx) ctx->err = msg;
    return AMX_E_BADARG;
}

// grow-only device workspace
static inline int amx_ensure(amx_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap && b.p) return AMX_OK;
    if (b.p) HIPCHK(ctx, hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    const size_t want = bytes + bytes / 8 + 256;
    HIPCHK(ctx, hipMalloc(&b.p, want));
    b.cap = want;
    return AMX_OK;
}

// misc buffer layout (ints): [0] n_chunks, [4..6] overflow counters of the 3 stages,
// [12] voxels that did not fit the large-MAXP variant either
struct Plan {
    int *lutidx, *perm, *counts, *dir_start, *cursor, *n_chunks, *ovf_count, *ovf_list;
    amx::Chunk *chunks;
    int max_chunks;
    size_t n;
    amx::Chunk *schunks = nullptr;  // larger chunks of the seed solver (count at n_chunks[1]); null: none
    int max_schunks = 0;
    int seed_chunk = 4096;         // voxels of one orientation per workgroup of the lane kernels (second plan)
    int seed1_waves = 4;           // the same for k_nnls_seed<1> (one wavefront per SIMD: with few voxels per chunk two wavefronts per workgroup keep more lanes busy)
    bool seed_occ2 = false, seed2_occ2 = false;   // k_nnls_seed<1> / k_lasso_seed in their two-wavefronts-per-SIMD builds (large calls)
    int seed2_waves = 4;           // wavefronts per workgroup of k_lasso_seed
    int seed_waves = 4;            // wavefronts per workgroup of the lane-per-voxel NODDI kernels (one workgroup per chunk of the second plan)
    int *feed = nullptr;           // kFeedSets sets of max_schunks + 8 chunk counters, one per kernel that shares its chunks (zeroed with the plan)
    int *feed_set(int k) const { return feed + (size_t)k * (max_schunks + 8); }
    // per-chunk counts of the lists the kernels of the chain compact (left-over lists of every certificate pass, clipped lists): one
    // array per pass, all in the arena behind the feed sets and cleared by the ONE memset that clears those -- each pass used to clear
    // its own (ten 5 us fill kernels per fit: 3 % of a 50 000-voxel call)
    int *zcount(int k) const { return feed + (size_t)(kFeedSetsN + k) * (max_schunks + 8); }
    static constexpr int kFeedSetsN = 7;
};
enum { FEED_SEED1 = 0, FEED_SEED2, FEED_SEED3, FEED_GEMM, FEED_CERT1, FEED_CERT2, FEED_CERT3, kFeedSets };
// (ZC_*, the arrays of Plan::zcount: amx_noddi_route.hpp)
static_assert(kFeedSets == Plan::kFeedSetsN, "Plan::zcount sits behind the feed sets");

// AMX_DEBUG=1: synchronise after every launch and trace progress on stderr
#define AMX_TRACE(ctx, s, what)                                                                   \
    do {                                                                                          \
        if ((ctx)->opt_debug) {                                                                   \
            fprintf(stderr, "[amx] %s ...", what); fflush(stderr);                                \
            hipError_t e_ = hipStreamSynchronize(s);                                              \
            fprintf(stderr, " %s\n", hipGetErrorString(e_)); fflush(stderr);                      \
        }                                                                                         \
    } while (0)

static inline void rec(amx_ctx *ctx, int k, hipStream_t s)
{
    // (an event in the stream is a packet of its own: ~5 us of a call's time each -- twenty of them 70 us of a 1.3 ms fit)
    if (ctx->profiling == 1 || (ctx->profiling >= 2 && (k < 2 ? 0 : k / 2) == ctx->profiling - 2)) { (void)hipEventRecord(ctx->ev[k], s); ctx->ev_valid[k] = true; }
}

// defined in the per-model launch units (amx_noddi.hip, amx_fw.hip, amx_sandi.hip)
int amx_build_basis(amx_ctx *ctx, amx_lut *lut);
// the NODDI launchers follow the fit's route (amx_noddi_route.hpp: noddi_fit_dev computes it once); none decides anything itself
inline amx::NoddiShape noddi_shape(const amx_lut *l)
{
    return {l->nS, l->ldA, l->n_atoms, l->n_wm, l->n_dwi, l->ndirs, l->is_exvivo, l->s2_derive,
            {l->basis_S != nullptr, l->gram != nullptr, l->gram_dwi != nullptr, l->basis2_S != nullptr, l->screen2_S != nullptr && l->screen2_kappa0 != nullptr && l->u2iso != nullptr}};
}
int amx_launch_noddi_project(amx_ctx *ctx, const amx_lut *lut, const amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiRoute &rt);
int amx_launch_noddi_seed(amx_ctx *ctx, const amx_lut *lut, const amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiRoute &rt, int stage);
int amx_launch_noddi_gcert(amx_ctx *ctx, const amx_lut *lut, const amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiRoute &rt, int stage, size_t *list_off, const int **count_out);
int amx_launch_noddi_gemm(amx_ctx *ctx, const amx_lut *lut, const amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiRoute &rt, bool lasso);
int amx_launch_noddi_s2prep(amx_ctx *ctx, const amx_lut *lut, const amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiRoute &rt);
int amx_launch_noddi_gcert2(amx_ctx *ctx, const amx_lut *lut, const amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiRoute &rt);
static inline size_t amx_rlist_half(const Plan &pl) { return (size_t)pl.n + pl.max_schunks + 64; }   // ints per left-over list + counts
int amx_launch_noddi_seed2(amx_ctx *ctx, const amx_lut *lut, const amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiRoute &rt);
int amx_launch_noddi_big(amx_ctx *ctx, const amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const int *list, const int *count, int n_all);   // amx_big.hip: LASSO stage, any support size
int amx_launch_noddi_s1(amx_ctx *ctx, amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiKernel &k);
int amx_launch_noddi_s2(amx_ctx *ctx, amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiKernel &k);
int amx_launch_noddi_s3(amx_ctx *ctx, amx::NoddiArgs &a, const Plan &pl, hipStream_t s, const amx::NoddiKernel &k);
// FreeWater, SANDI and CylinderZeppelinBall follow the fit's route too (amx_small_route.hpp: amx_fit_dev computes it once)
inline amx::SmallShape small_shape(const amx_lut *l) { return {l->model, l->nS, l->ldA, l->n_atoms, l->ndirs, l->gram != nullptr}; }
inline amx::SmallSwitches small_switches(const amx_ctx *c) { return {c->opt_wave_per_voxel, c->opt_no_refill, c->opt_sandi_atom_space, c->opt_fw_no_fuse}; }
int amx_launch_fw(amx_ctx *ctx, amx::FwArgs &a, const Plan &pl, hipStream_t s, const amx::SmallRoute &rt);
int amx_launch_sandi(amx_ctx *ctx, amx::SandiArgs &a, const Plan &pl, hipStream_t s, const amx::SmallRoute &rt);
int amx_launch_czb(amx_ctx *ctx, amx::CzbArgs &a, const Plan &pl, hipStream_t s, const amx::SmallRoute &rt);
int amx_launch_batched(amx_ctx *ctx, amx::BatchedArgs &a, const Plan &pl, hipStream_t s, bool ridge, bool dense = false);
int amx_launch_batched_big(amx_ctx *ctx, const amx::BatchedArgs &a, const amx_dict *dict, const Plan &pl, hipStream_t s);   // amx_batched_big.hip: a dense dictionary's voxels beyond 48 atoms
int amx_build_dict_gram(amx_ctx *ctx, const amx_dict *dict);                                                              // ... and its Gram tables
// FreeWater, SANDI and CylinderZeppelinBall on dictionaries of kSmallMaxAtoms + 1 .. kBigMaxAtoms atoms (amx_enet_big.hip): the Gram tables made at
// the upload, and k_enet_big -- a workgroup per voxel, in bucket order (SANDI: the voxels in order)
static inline bool amx_big_dictionary(const amx_lut *lut) { return lut->n_atoms > amx::kSmallMaxAtoms; }      // (the upload's question; a fit asks its route)
int amx_build_big_gram(amx_ctx *ctx, amx_lut *lut);
int amx_launch_enet_big(amx_ctx *ctx, const amx_lut *lut, const amx::FwArgs &a, const Plan &pl, int64_t n, hipStream_t s, const amx::SmallRoute &rt);
int amx_launch_enet_big(amx_ctx *ctx, const amx_lut *lut, const amx::SandiArgs &a, int64_t n, hipStream_t s, const amx::SmallRoute &rt);
int amx_launch_enet_big(amx_ctx *ctx, const amx_lut *lut, const amx::CzbArgs &a, const Plan &pl, int64_t n, hipStream_t s, const amx::SmallRoute &rt);
// the per-dictionary tables a route names (SmallRoute::tables), cached in the dictionary handle for one lambda2 (SANDI's row-space tables: lambda1 too)
int amx_fw_prepare(amx_ctx *ctx, const amx_lut *lut, amx::FwArgs &a, hipStream_t s, const amx::SmallRoute &rt);
int amx_sandi_prepare(amx_ctx *ctx, const amx_lut *lut, amx::SandiArgs &a, hipStream_t s);
int amx_sandi_long_prepare(amx_ctx *ctx, const amx_lut *lut, double lam2, hipStream_t s);
int amx_czb_prepare(amx_ctx *ctx, const amx_lut *lut, double lam2, hipStream_t s, const amx::SmallRoute &rt);
// doubles of those tables (per orientation where the model has orientations): amx_debug_fetch
size_t amx_czb_table_stride(int nS);
size_t amx_fw_table_words(const amx_lut *lut);
size_t amx_sandi_table_words();
size_t amx_sandi_long_table_words(const amx_lut *lut);
int amx_launch_czb_fast(amx_ctx *ctx, const amx_lut *lut, amx::CzbArgs &a, const Plan &pl, hipStream_t s, const amx::SmallRoute &rt);
// lane-per-voxel variants for dictionaries of <= 16 atoms (amx_fw_lane.hip, amx_sandi_lane.hip)
int amx_launch_fw_small(amx_ctx *ctx, amx::FwArgs &a, const Plan &pl, hipStream_t s, const amx::SmallRoute &rt);
int amx_launch_sandi_small(amx_ctx *ctx, amx::SandiArgs &a, const Plan &pl, hipStream_t s, const amx::SmallRoute &rt);
// SANDI, protocols of more than kSandiShortNS volumes (amx_sandi_long.hip): projection on the matrix cores, then a Gram-space solver
int amx_launch_sandi_long(amx_ctx *ctx, const amx_lut *lut, const amx::SandiArgs &a, int64_t n, hipStream_t s, const amx::SmallRoute &rt);

// ------------------------------------------------------------------ what the entry-point units share (library-internal: not exported)
#pragma GCC visibility push(hidden)
// One row per model: what the shared prologue / epilogue of a fit needs to know
struct FitSpec {
    int model;                     // amx_lut::model
    const char *name, *what;       // in messages: "<name>: not a <what> dictionary"
    bool dirs;                     // takes DIRs (a plan by orientation); SANDI has one dictionary
    int maps;                      // per voxel (+ 1 for an ex-vivo NODDI dictionary, + 2 for FreeWater's Mouse)
    unsigned extra_flag;           // the flag of the optional fourth output (0: none), its columns (0: the dictionary's nS)
    int extra_cols;
    int x_per_atom;                // coefficients per atom and voxel that AMX_F_DEBUG_X stores
    unsigned model_flags;          // flags only this model's fit takes (FreeWater: AMX_F_FW_ISO); on any other model's they are AMX_E_BADARG
};
extern const FitSpec kFits[4];     // by model - 1 (amx_fit_dev.hip)
inline int fit_bad(amx_ctx *ctx, const FitSpec &m, const char *a, const char *b = nullptr) { return amx_bad(ctx, (std::string(m.name) + a + (b ? m.what : "") + (b ? b : "")).c_str()); }

// the arguments of one device fit, whichever the model (y or y32 is set; extra: NODDI's modulated maps / FreeWater's corrected DWI)
struct FitCall {
    const amx_lut *lut; const double *y; const float *y32; const double *dirs; int64_t n;
    double lam1, lam2; int is_mouse; unsigned flags;
    double *est, *rmse, *nrmse, *extra; hipStream_t stream;
    Batch batch;
};
inline int fit_maps(const FitSpec &m, const FitCall &c) { return m.maps + (c.lut->is_exvivo ? 1 : 0) + (c.is_mouse ? 2 : 0); }
int amx_fit_dev(amx_ctx *ctx, const FitSpec &spec, FitCall c);                     // amx_fit_dev.hip

// the ONE place that fills the arguments every solver kernel shares (the overflow lists are launch_pair's)
inline void fill_common(amx::FitCommon &c, const void *tiles, const double *y, const float *y32, const Plan &pl, int *status, int nS, int ldA,
                        int n_atoms, int tile_stride, double lam1, double lam2, unsigned flags)
{
    c.tiles = tiles; c.y = y; c.y32 = y32; c.perm = pl.perm; c.chunks = pl.chunks; c.n_chunks = pl.n_chunks;
    c.lutidx = pl.lutidx; c.status = status; c.nS = nS; c.ldA = ldA;
    c.n_atoms = n_atoms; c.tile_stride = tile_stride; c.lam1 = lam1; c.lam2 = lam2; c.flags = flags;
}

// amx_plan.hip: the per-call plan and the small launches around the solvers
int make_plan(amx_ctx *ctx, int64_t n, int ndirs, Plan &pl, const amx::NoddiRoute *seeds = nullptr, int table_rows = 0, int blocks_chunk = 0);   // seeds: a NODDI fit on the seeded chain, its route
int enqueue_bucketing(amx_ctx *ctx, const amx_lut *lut, const double *d_dirs, int64_t n, Plan &pl, hipStream_t s, int chunk = kChunk,
                      double *zero_rows = nullptr, int zero_cols = 0, double *zero_rows2 = nullptr, int zero_cols2 = 0);
int enqueue_index_bucketing(amx_ctx *ctx, const int32_t *d_idx, int n_dicts, int64_t n, Plan &pl, hipStream_t s);   // the batched solvers' plan
int enqueue_linear_plan(amx_ctx *ctx, int64_t n, Plan &pl, hipStream_t s);                                          // SANDI's: the voxels in order
int enqueue_dir_to_lut(amx_ctx *ctx, const amx_lut *lut, const double *d_dirs, int64_t n, int *d_idx, hipStream_t s);              // the LUT indices alone (amx_predict.hip)
void fold_counters(amx_ctx *ctx, hipStream_t s);
void widen_on_device(const float *d_y32, double *dst, size_t nel, hipStream_t s);
void clear_events(amx_ctx *ctx);
void progress_tick(amx_ctx *ctx, hipStream_t s, int64_t done, int64_t total);
// amx_fit_host.hip: the host threads of the float32 transport are made beside a dictionary upload
void prefetch_stage_pool(amx_ctx *ctx);

template <typename T>
static int amx_upload(amx_ctx *ctx, T **dst, const T *src, size_t n)
{
    HIPCHK(ctx, hipMalloc((void **)dst, n * sizeof(T) + 16));
    HIPCHK(ctx, hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return AMX_OK;
}
#define AMX_H2D(buf, src, bytes)                                                     \
    if ((rc = amx_ensure(ctx, buf, bytes))) return rc;                               \
    HIPCHK(ctx, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, nullptr));
#pragma GCC visibility pop
