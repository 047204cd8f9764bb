// amx_fit_dev.hip -- the four model fits on device pointers.  One checked, prepared call (fit_check, fit_open, fit_args, fit_close) around
// what is a model's own: NODDI's chain of three stages; FreeWater, SANDI and CylinderZeppelinBall as their route says (amx_small_route.hpp).
#include "amx_host.hpp"

using namespace amx;

// (CylinderZeppelinBall: the Gram-space solver needs a ridge -- models.pyx:439 default: 4.0; lambda2 < 1e-6 runs the thin-QR solver in A-space)
const FitSpec kFits[4] = {{1, "amx_noddi_fit", "NODDI", true, 3, AMX_F_MODULATED, 2, 3, 0}, {2, "amx_freewater_fit", "FreeWater", true, 2, AMX_F_CORRECTED, 0, 1, AMX_F_FW_ISO},
                          {3, "amx_sandi_fit", "SANDI", false, 6, 0, 1, 1, 0}, {4, "amx_czb_fit", "CylinderZeppelinBall", true, 3, 0, 1, 1, 0}};
constexpr unsigned kModelFlags = AMX_F_FW_ISO;       // every flag that belongs to one model (FitSpec::model_flags)

namespace {

// ------------------------------------------------------------------ the prologue and epilogue every fit shares
// The checks, in the order they have always run; then the context learns where this fit stands in its call (amx_note, progress_tick,
// enqueue_bucketing and every size-dependent path choice read it from there).  A call of no voxels passes: amx_fit_dev returns AMX_OK.
int fit_check(amx_ctx *ctx, const FitSpec &m, const FitCall &c)
{
    if (ctx && c.batch.first()) ctx->path.clear();
    if (!ctx) return AMX_E_BADARG;
    if (!c.lut || c.lut->model != m.model || c.lut->ctx != ctx) return fit_bad(ctx, m, ": not a ", " dictionary of this ctx");
    if (c.n < 0 || c.n > INT_MAX / 4) return fit_bad(ctx, m, ": bad n_vox");
    if (c.n == 0) return AMX_OK;
    if ((!c.y && !c.y32) || (m.dirs && !c.dirs) || !c.est) return fit_bad(ctx, m, ": null buffer");
    if (((c.flags & AMX_F_RMSE) && !c.rmse) || ((c.flags & AMX_F_NRMSE) && !c.nrmse) || ((c.flags & m.extra_flag) && !c.extra)) return fit_bad(ctx, m, ": flag set but output buffer is null");
    if (c.flags & kModelFlags & ~m.model_flags) return fit_bad(ctx, m, ": AMX_F_FW_ISO is a flag of the FreeWater fit");
    if ((c.flags & m.model_flags & AMX_F_FW_ISO) && !ctx->fw_iso) return fit_bad(ctx, m, ": AMX_F_FW_ISO without a buffer (amx_set_fw_iso)");
    if (!(c.lam2 >= 0.0) || !(c.lam1 >= 0.0)) return fit_bad(ctx, m, ": need lambda1 >= 0 and lambda2 >= 0");
    if (c.is_mouse && c.lut->n_iso < 2) return amx_bad(ctx, "amx_freewater_fit: Mouse needs two isotropic atoms");   // (is_mouse: FreeWater only)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->batch = c.batch;
    ctx->call_vox = c.batch.call_vox > 0 ? c.batch.call_vox : c.n;
    return AMX_OK;
}

// the call's first event, and the voxels bucketed by orientation (a voxel whose direction is out of bounds is skipped by every kernel:
// k_dir_to_lut gives it defined (zero) maps, so no fit clears its maps first -- test_*_fit_writes_every_voxel)
int fit_open(amx_ctx *ctx, const FitSpec &m, const FitCall &c, Plan &pl, int chunk = kChunk, double *zero_rows2 = nullptr, int zero_cols2 = 0)
{
    clear_events(ctx);
    rec(ctx, 0, c.stream);
    return m.dirs ? enqueue_bucketing(ctx, c.lut, c.dirs, c.n, pl, c.stream, chunk, c.est, fit_maps(m, c), zero_rows2, zero_cols2) : AMX_OK;
}

// what every model's kernel arguments have in common; the outputs are gated by their flags
template <typename Args>
int fit_args(amx_ctx *ctx, const FitSpec &m, const FitCall &c, const Plan &pl, Args &a, double *Args::*extra = nullptr)
{
    const amx_lut *lut = c.lut;
    memset(&a, 0, sizeof a);
    fill_common(a.c, lut->tiles, c.y, c.y32, pl, ctx->status_d, lut->nS, lut->ldA, lut->n_atoms, lut->tile_stride, c.lam1, c.lam2, c.flags);
    if (c.flags & AMX_F_DEBUG_X) {
        if (!ctx->dbg_x) return fit_bad(ctx, m, ": AMX_F_DEBUG_X without a buffer (amx_set_debug_x)");
        a.c.xdbg = ctx->dbg_x + (size_t)c.batch.base * m.x_per_atom * lut->n_atoms;
    }
    a.est = c.est; a.rmse = (c.flags & AMX_F_RMSE) ? c.rmse : nullptr; a.nrmse = (c.flags & AMX_F_NRMSE) ? c.nrmse : nullptr;
    if (extra) a.*extra = (c.flags & m.extra_flag) ? c.extra : nullptr;
    return AMX_OK;
}

// (fold: the kernels counted into the per-call counters.  A failed launch still ends the call's event pair: rc is what the solver launch gave)
int fit_close(amx_ctx *ctx, const FitCall &c, int rc, bool fold = true)
{
    if (fold) fold_counters(ctx, c.stream);
    rec(ctx, 1, c.stream);
    if (!rc) progress_tick(ctx, c.stream, c.n, c.n);
    return rc;
}

// ------------------------------------------------------------------ NODDI
// What the three stages share.  Every stage is: [seed solver -> Gram certificate ->] the stage's wavefront-per-voxel kernel, which works
// on all voxels of the first plan (walk_all) or, behind a certificate, on the lists that certificate left over (walk_leftovers).
struct NoddiChain {
    amx_ctx *ctx; const amx_lut *lut; int64_t n; hipStream_t s;
    Plan pl; NoddiArgs a;
    NoddiRoute rt;                 // every choice of kernel build of this fit (amx_noddi_route.hpp), made once in noddi_fit_dev
    // AMX_FORK (a recorded negative result, kSwitches): the side stream and its events, what went there
    hipStream_t fs = nullptr; hipEvent_t *fev = nullptr;
    bool joined1 = false;
    int late_rc = AMX_OK;          // of the LASSO stage's own launch: the epilogue still runs behind it, as it always has
};

// the stage kernel walks the left-over lists of the second plan
void walk_leftovers(NoddiChain &q, const int *list, const int *counts, const unsigned char *done)
{
    q.a.done = done; q.a.rlist = list; q.a.rcount = counts;
    q.a.c.chunks = q.pl.schunks; q.a.c.n_chunks = q.pl.n_chunks + 1;
}

// ... back to all voxels of the first plan
void walk_all(NoddiChain &q)
{
    q.a.c.chunks = q.pl.chunks; q.a.c.n_chunks = q.pl.n_chunks;
    q.a.rlist = nullptr; q.a.rcount = nullptr; q.a.done = nullptr;
}

// side stream + events of a forked fit, one set per workspace set (fit_host alternates two: swap_work)
int fork_ready(NoddiChain &q)
{
    amx_ctx *ctx = q.ctx; const int w = ctx->work_idx;
    if (!ctx->fork_s[w]) {
        HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->fork_s[w], hipStreamNonBlocking, 0));
        for (int k = 0; k < 4; k++) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->fork_ev[w][k], hipEventDisableTiming));
    }
    q.fs = ctx->fork_s[w];
    return AMX_OK;
}

// what `launch` enqueues runs on the side stream, behind everything the main stream holds so far: events ev (fork) and ev + 1 (done)
template <typename Launch>
int fork_side(NoddiChain &q, int ev, Launch launch)
{
    amx_ctx *ctx = q.ctx;
    HIPCHK(ctx, hipEventRecord(q.fev[ev], q.s));
    HIPCHK(ctx, hipStreamWaitEvent(q.fs, q.fev[ev], 0));
    ctx->side_launch = true;
    const int rc = launch(q.fs);
    ctx->side_launch = false;
    if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(q.fev[ev + 1], q.fs));
    return AMX_OK;
}

int fork_join(NoddiChain &q, int ev)
{
    HIPCHK(q.ctx, hipStreamWaitEvent(q.s, q.fev[ev + 1], 0));
    return AMX_OK;
}

// NNLS on all atoms: x_iso (and x_dot)
int noddi_stage1(NoddiChain &q)
{
    amx_ctx *ctx = q.ctx; const amx_lut *lut = q.lut; NoddiArgs &a = q.a; const Plan &pl = q.pl; hipStream_t s = q.s; const NoddiRoute &rt = q.rt; int rc;
    if (rt.seeds) {
        ctx->seeded_vox += q.n;
        // y~ = U'y once; the seed solver proposes the stage's support, the stage kernel certifies it (amx_seed.hpp)
        rec(ctx, 10, s);
        const bool gcert = rt.gcert;
        if (gcert && (rc = amx_launch_noddi_gemm(ctx, lut, a, pl, s, rt, false))) return rc;
        if (!gcert && (rc = amx_launch_noddi_project(ctx, lut, a, pl, s, rt))) return rc;      // (the GEMM writes y~ as well)
        if (!ctx->opt_no_screen) { a.scr_S = lut->screen_S; a.scr_kappa = lut->screen_kappa; a.scr_ytil = (const double *)ctx->ytil.p; a.scr_Sg = lut->basis_S; }
        if (rt.seed1) {
            a.seeds = (const unsigned long long *)ctx->seeds.p;
            rec(ctx, 16, s);
            if ((rc = amx_launch_noddi_seed(ctx, lut, a, pl, s, rt, 1))) return rc;
            rec(ctx, 17, s);
            if (!gcert) ctx->uncert_vox[0] += q.n;
            if (gcert) {
                size_t off = 0; const int *cnt = nullptr;
                if ((rc = amx_launch_noddi_gcert(ctx, lut, a, pl, s, rt, 1, &off, &cnt))) return rc;
                walk_leftovers(q, (const int *)ctx->rlist.p + off, cnt, ctx->opt_no_hard_first ? nullptr : (const unsigned char *)ctx->done.p);
            }
        }
        rec(ctx, 11, s);
    }
    // AMX_FORK bit 0 (TIMING PROBE, not a fit): the stage-1 left-over kernel on the side stream beside the LASSO seed solver, which reads
    // the x_iso the previous call left for those voxels; joined before the LASSO certificates
    if (ctx->opt_fork && (rc = fork_ready(q))) return rc;
    q.fev = ctx->fork_ev[ctx->work_idx];
    if (rt.fork1) rc = fork_side(q, 0, [&](hipStream_t side) { return amx_launch_noddi_s1(ctx, a, pl, side, rt.s1); });
    else rc = amx_launch_noddi_s1(ctx, a, pl, s, rt.s1);
    if (rc) return rc;
    progress_tick(ctx, s, q.n / 3, q.n);                       // (three stages: a third of the work each, roughly)
    walk_all(q);
    return AMX_OK;
}

// LASSO on the white-matter atoms: the support
int noddi_stage2(NoddiChain &q)
{
    amx_ctx *ctx = q.ctx; const amx_lut *lut = q.lut; NoddiArgs &a = q.a; const Plan &pl = q.pl; hipStream_t s = q.s; const NoddiRoute &rt = q.rt; int rc;
    if (rt.seeds2) {       // (the LASSO seeds need x_iso: Gram-space solver only)
        const bool gcert2 = rt.gcert2;
        rec(ctx, 12, s);
        // y2~ of every voxel and c2 = A2'y2, ||y2||^2 of the unclipped ones derive from the stage-1 table; the clipped voxels' exactly
        if (gcert2 && (rc = amx_launch_noddi_s2prep(ctx, lut, a, pl, s, rt))) return rc;
        rec(ctx, 18, s);
        if ((rc = amx_launch_noddi_seed2(ctx, lut, a, pl, s, rt))) return rc;
        rec(ctx, 19, s);
        a.seeds2 = (const unsigned long long *)ctx->seeds2.p;
        a.list_is_pos = 1;
        if (!ctx->opt_no_screen && lut->screen2_S) { a.scr2_S = lut->screen2_S; a.scr2_kappa = lut->screen2_kappa; a.scr2_ytil = (const double *)ctx->ytil2.p; a.scr2_Sg = lut->basis2_S; }
        if (!gcert2) ctx->uncert_vox[1] += q.n;
        if (rt.fork1) { if ((rc = fork_join(q, 0))) return rc; q.joined1 = true; }
        if (gcert2) {
            if ((rc = amx_launch_noddi_gcert2(ctx, lut, a, pl, s, rt))) return rc;
            a.cand_lists = 1;       // (k_lasso_gcert: the candidate lists of stage 3 wait in seeds2 for the voxels it settled)
            walk_leftovers(q, (const int *)ctx->rlist.p + (rt.left2_second_half ? amx_rlist_half(pl) : 0), pl.zcount(rt.left2_count), nullptr);
            // AMX_FORK bit 1: the voxels these certificates left over (0.6 %) do not come back to the lane kernels -- k_noddi<4> and then
            // k_noddi<3> (no seed: Lawson-Hanson on the support it has just found, plus iso) finish them, a wavefront per voxel, on the side
            // stream, while k_nnls_seed<3> / k_nnls_gcert<3> work on everybody else (they skip the voxels whose certificate flag is not 1): rt.fork2
        }
        rec(ctx, 13, s);
    }
    if (rt.fork1 && !q.joined1 && (rc = fork_join(q, 0))) return rc;
    if (!rt.fork2) { q.late_rc = amx_launch_noddi_s2(ctx, a, pl, s, rt.s2); return AMX_OK; }
    rc = fork_side(q, 2, [&](hipStream_t side) {
        NoddiArgs b = a;
        int r = amx_launch_noddi_s2(ctx, b, pl, side, rt.s2);
        if (r) return r;
        b = a;      // (same left-over lists, same chunks: now stage 3 without seeds)
        b.seeds = nullptr; b.done = nullptr; b.seeds2 = nullptr; b.cand_lists = 0;
        return amx_launch_noddi_s3(ctx, b, pl, side, rt.s3_fork);
    });
    if (!rc) a.fork_l2 = 1;
    return rc;
}

// NNLS on the support + iso: the maps
int noddi_stage3(NoddiChain &q)
{
    amx_ctx *ctx = q.ctx; const amx_lut *lut = q.lut; NoddiArgs &a = q.a; const Plan &pl = q.pl; hipStream_t s = q.s; const NoddiRoute &rt = q.rt; int rc = AMX_OK;
    progress_tick(ctx, s, 2 * (q.n / 3), q.n);
    a.seeds = nullptr;
    walk_all(q);
    if (rt.seed3) {
        a.seeds = (const unsigned long long *)ctx->seeds.p;
        rec(ctx, 14, s);
        rc = amx_launch_noddi_seed(ctx, lut, a, pl, s, rt, 3);
        const bool gcert3 = rt.gcert;
        if (!gcert3) ctx->uncert_vox[2] += q.n;
        if (!rc && gcert3) {
            size_t off = 0; const int *cnt = nullptr;
            rc = amx_launch_noddi_gcert(ctx, lut, a, pl, s, rt, 3, &off, &cnt);
            walk_leftovers(q, (const int *)ctx->rlist.p + off, cnt, ctx->opt_no_hard_first ? nullptr : (const unsigned char *)ctx->done.p);
        }
        rec(ctx, 15, s);
    }
    return rc ? rc : amx_launch_noddi_s3(ctx, a, pl, s, rt.s3);
}

int noddi_fit_dev(amx_ctx *ctx, const FitSpec &m, const FitCall &c)
{
    const amx_lut *lut = c.lut; int rc;
    NoddiChain q{ctx, lut, c.n, c.stream};
    q.rt = noddi_route(noddi_shape(lut), {c.n, ctx->call_vox, c.lam1, c.lam2}, noddi_switches(ctx));      // (fit_check has set ctx->call_vox)
    if ((rc = make_plan(ctx, c.n, lut->ndirs, q.pl, q.rt.seeds ? &q.rt : nullptr, gemm_rows(lut->n_atoms)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->xiso, (size_t)c.n * 2 * sizeof(double)))) return rc;
    if ((rc = amx_ensure(ctx, ctx->supp, (size_t)c.n * 4 * sizeof(unsigned long long)))) return rc;
    // (every voxel's maps are written by the kernel that settles its stage 3 -- tests/test_gpu_parity.py::test_noddi_fit_writes_every_voxel)
    if ((rc = fit_open(ctx, m, c, q.pl)) || (rc = fit_args(ctx, m, c, q.pl, q.a, &NoddiArgs::mod))) return rc;
    NoddiArgs &a = q.a;
    a.rowdwi = lut->rowdwi; a.colscale = lut->colscale; a.icvf = lut->icvf; a.kappa = lut->kappa;
    a.n_wm = lut->n_wm; a.is_exvivo = lut->is_exvivo; a.n_maps = fit_maps(m, c);
    a.gram = lut->gram; a.gram_dwi = lut->gram_dwi; a.ldG = lut->ldG;
    a.xiso = (double *)ctx->xiso.p; a.supp = (unsigned long long *)ctx->supp.p;
    if ((rc = noddi_stage1(q)) || (rc = noddi_stage2(q))) return rc;      // (a failure up to the LASSO certificates leaves the call at once)
    // the launch of the LASSO stage's own kernels on the main stream reports through late_rc: behind it the counters still fold and the call's
    // event pair still ends (fit_close), so a profiled or polled call sees a finished call and the error, as it always has
    rc = q.late_rc ? q.late_rc : noddi_stage3(q);
    if (q.rt.fork2) { const int rj = fork_join(q, 2); if (rj) return rj; }      // the side stream's voxels are part of this fit
    return fit_close(ctx, c, rc);
}

// ------------------------------------------------------------------ FreeWater, SANDI, CylinderZeppelinBall: each follows its route (amx_small_route.hpp)
int freewater_fit_dev(amx_ctx *ctx, const FitSpec &m, const FitCall &c, const SmallRoute &rt)
{
    const amx_lut *lut = c.lut; hipStream_t s = c.stream; Plan pl; int rc;
    if ((rc = make_plan(ctx, c.n, lut->ndirs, pl))) return rc;
    FwArgs a;
    // AMX_F_FW_ISO: the isotropic coefficients of every voxel, at the voxel's index in the caller's buffer (fit_check has seen the buffer)
    double *xiso = (c.flags & AMX_F_FW_ISO) ? ctx->fw_iso + (size_t)c.batch.base * lut->n_iso : nullptr;
    if ((rc = fit_open(ctx, m, c, pl, rt.chunk, xiso, lut->n_iso)) || (rc = fit_args(ctx, m, c, pl, a, &FwArgs::ycorr))) return rc;
    a.n_perp = lut->n_perp; a.n_iso = lut->n_iso; a.is_mouse = c.is_mouse; a.n_maps = fit_maps(m, c); a.xiso = xiso;
    if (rt.tables == SMT_FW && (rc = amx_fw_prepare(ctx, lut, a, s, rt))) return rc;
    return fit_close(ctx, c, rt.family == SF_ENET_BIG ? amx_launch_enet_big(ctx, lut, a, pl, c.n, s, rt) : amx_launch_fw(ctx, a, pl, s, rt));
}

int sandi_fit_dev(amx_ctx *ctx, const FitSpec &m, const FitCall &c, const SmallRoute &rt)
{
    const amx_lut *lut = c.lut; hipStream_t s = c.stream; Plan pl; int rc;
    if ((rc = make_plan(ctx, c.n, 1, pl))) return rc;
    SandiArgs a;
    if ((rc = fit_open(ctx, m, c, pl)) || (rc = fit_args(ctx, m, c, pl, a))) return rc;      // (one dictionary: no bucketing)
    a.norms = lut->norms; a.Rs = lut->Rs; a.d_in = lut->d_in; a.d_isos = lut->d_isos;
    a.n_rs = lut->n_rs; a.n_in = lut->n_in; a.n_iso = lut->n_isos;
    if (rt.tables == SMT_SANDI && (rc = amx_sandi_prepare(ctx, lut, a, s))) return rc;
    if (rt.tables == SMT_SANDI_LONG && (rc = amx_sandi_long_prepare(ctx, lut, c.lam2, s))) return rc;
    // the voxels in order (k_enet_big, the long protocols' kernels, the row-space kernel): they count straight into the status words;
    // the other SANDI kernels walk the (trivial) plan and use the per-call counters
    if (rt.family == SF_SANDI_ROWS) a.n_lin = (int)c.n;
    if (!rt.in_order && (rc = enqueue_linear_plan(ctx, c.n, pl, s))) return rc;
    switch (rt.family) {
    case SF_ENET_BIG: rc = amx_launch_enet_big(ctx, lut, a, c.n, s, rt); break;
    case SF_SANDI_LONG_LANE: case SF_SANDI_LONG_WAVE: rc = amx_launch_sandi_long(ctx, lut, a, c.n, s, rt); break;
    default: rc = amx_launch_sandi(ctx, a, pl, s, rt);
    }
    return fit_close(ctx, c, rc, !rt.in_order);
}

int czb_fit_dev(amx_ctx *ctx, const FitSpec &m, const FitCall &c, const SmallRoute &rt)
{
    const amx_lut *lut = c.lut; hipStream_t s = c.stream; Plan pl; int rc;
    if ((rc = make_plan(ctx, c.n, lut->ndirs, pl, nullptr, 64, rt.blocks_chunk))) return rc;
    CzbArgs a;
    if ((rc = fit_open(ctx, m, c, pl)) || (rc = fit_args(ctx, m, c, pl, a))) return rc;
    a.n_rs = lut->n_rs; a.n_perp = lut->n_perp; a.Rs = lut->Rs; a.gram = lut->gram; a.ldG = lut->ldG;
    if (rt.family == SF_CZB_FAST) { if (!(rc = amx_czb_prepare(ctx, lut, c.lam2, s, rt))) rc = amx_launch_czb_fast(ctx, lut, a, pl, s, rt); }
    else rc = rt.family == SF_ENET_BIG ? amx_launch_enet_big(ctx, lut, a, pl, c.n, s, rt) : amx_launch_czb(ctx, a, pl, s, rt);
    return fit_close(ctx, c, rc);
}

}  // namespace

// The argument checks, then -- for the three small models -- the fit's route, once: a shape it refuses leaves here before anything is enqueued
// (with the launches the fit had noted when it used to find out); float32 signals in HBM (the image's dtype, core.py:136; lossless) get a
// float64 copy made on the device first where the route's kernels read float64 only.  (The NODDI kernels read either: noddi_fit_dev.)
int amx_fit_dev(amx_ctx *ctx, const FitSpec &m, FitCall c)
{
    int rc;
    if ((rc = fit_check(ctx, m, c)) || c.n == 0) return rc;
    if (m.model == 1) return noddi_fit_dev(ctx, m, c);
    const SmallRoute rt = small_route(small_shape(c.lut), {c.n, c.lam1, c.lam2, c.flags, c.y32 != nullptr}, small_switches(ctx));
    if (rt.refusal) {
        for (int l = 0; l < rt.n_launch; l++) amx_note(ctx, rt.launch[l]);
        return amx_bad(ctx, rt.error);
    }
    if (rt.widen) {
        const size_t nel = (size_t)c.n * c.lut->nS;
        if ((rc = amx_ensure(ctx, ctx->wy, nel * sizeof(double)))) return rc;
        widen_on_device(c.y32, (double *)ctx->wy.p, nel, c.stream);
        HIPCHK(ctx, hipGetLastError());
        c.y = (const double *)ctx->wy.p; c.y32 = nullptr;
    }
    switch (m.model) {
    case 2: return freewater_fit_dev(ctx, m, c, rt);
    case 3: return sandi_fit_dev(ctx, m, c, rt);
    default: return czb_fit_dev(ctx, m, c, rt);
    }
}

// ------------------------------------------------------------------ the C entry points: float64 signals, or the float32 the image holds
extern "C" {

int amx_noddi_fit_device(amx_ctx *ctx, const amx_lut *lut, const double *d_y, const double *d_dirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *d_estimates, double *d_rmse, double *d_nrmse, double *d_mod, void *hip_stream)
{
    return amx_fit_dev(ctx, kFits[0], {lut, d_y, nullptr, d_dirs, n_vox, lambda1, lambda2, 0, flags, d_estimates, d_rmse, d_nrmse, d_mod, (hipStream_t)hip_stream, {}});
}
int amx_noddi_fit_device_f32(amx_ctx *ctx, const amx_lut *lut, const float *d_y, const double *d_dirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *d_estimates, double *d_rmse, double *d_nrmse, double *d_mod, void *hip_stream)
{
    return amx_fit_dev(ctx, kFits[0], {lut, nullptr, d_y, d_dirs, n_vox, lambda1, lambda2, 0, flags, d_estimates, d_rmse, d_nrmse, d_mod, (hipStream_t)hip_stream, {}});
}

int amx_freewater_fit_device(amx_ctx *ctx, const amx_lut *lut, const double *d_y, const double *d_dirs, int64_t n_vox, double lambda1, double lambda2, int is_mouse, unsigned flags, double *d_estimates, double *d_rmse, double *d_nrmse, double *d_ycorr, void *hip_stream)
{
    return amx_fit_dev(ctx, kFits[1], {lut, d_y, nullptr, d_dirs, n_vox, lambda1, lambda2, is_mouse, flags, d_estimates, d_rmse, d_nrmse, d_ycorr, (hipStream_t)hip_stream, {}});
}
int amx_freewater_fit_device_f32(amx_ctx *ctx, const amx_lut *lut, const float *d_y, const double *d_dirs, int64_t n_vox, double lambda1, double lambda2, int is_mouse, unsigned flags, double *d_estimates, double *d_rmse, double *d_nrmse, double *d_ycorr, void *hip_stream)
{
    return amx_fit_dev(ctx, kFits[1], {lut, nullptr, d_y, d_dirs, n_vox, lambda1, lambda2, is_mouse, flags, d_estimates, d_rmse, d_nrmse, d_ycorr, (hipStream_t)hip_stream, {}});
}

int amx_sandi_fit_device(amx_ctx *ctx, const amx_lut *lut, const double *d_y, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *d_estimates, double *d_rmse, double *d_nrmse, void *hip_stream)
{
    return amx_fit_dev(ctx, kFits[2], {lut, d_y, nullptr, nullptr, n_vox, lambda1, lambda2, 0, flags, d_estimates, d_rmse, d_nrmse, nullptr, (hipStream_t)hip_stream, {}});
}
int amx_sandi_fit_device_f32(amx_ctx *ctx, const amx_lut *lut, const float *d_y, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *d_estimates, double *d_rmse, double *d_nrmse, void *hip_stream)
{
    return amx_fit_dev(ctx, kFits[2], {lut, nullptr, d_y, nullptr, n_vox, lambda1, lambda2, 0, flags, d_estimates, d_rmse, d_nrmse, nullptr, (hipStream_t)hip_stream, {}});
}

int amx_czb_fit_device(amx_ctx *ctx, const amx_lut *lut, const double *d_y, const double *d_dirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *d_estimates, double *d_rmse, double *d_nrmse, void *hip_stream)
{
    return amx_fit_dev(ctx, kFits[3], {lut, d_y, nullptr, d_dirs, n_vox, lambda1, lambda2, 0, flags, d_estimates, d_rmse, d_nrmse, nullptr, (hipStream_t)hip_stream, {}});
}
int amx_czb_fit_device_f32(amx_ctx *ctx, const amx_lut *lut, const float *d_y, const double *d_dirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, double *d_estimates, double *d_rmse, double *d_nrmse, void *hip_stream)
{
    return amx_fit_dev(ctx, kFits[3], {lut, nullptr, d_y, d_dirs, n_vox, lambda1, lambda2, 0, flags, d_estimates, d_rmse, d_nrmse, nullptr, (hipStream_t)hip_stream, {}});
}

}  // extern "C"
