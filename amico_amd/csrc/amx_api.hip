// amx_api.hip -- C ABI (include/amico_amd.h) of the MI355X-native AMICO fitter: the context and its switches, status, diagnostics.
// (dictionaries: amx_lut.hip; the fits: amx_fit_dev.hip, amx_fit_host.hip; the batched solvers: amx_batched.hip; the per-call plan: amx_plan.hip)
#include "amx_host.hpp"

using namespace amx;

namespace {

int reset_status(amx_ctx *ctx, hipStream_t s)
{
    HIPCHK(ctx, hipMemsetAsync(ctx->status_d, 0, ST_WORDS * sizeof(int), s));
    HIPCHK(ctx, hipMemsetAsync(ctx->status_d + ST_ERRPACK, 0x7f, 2 * sizeof(int), s));
    return AMX_OK;
}

// wavefront primitives exercised on the device (tests/test_gpu_parity.py::test_wave_primitives)
__global__ void k_selftest(double *out)
{
    const int lane = threadIdx.x & 63;
    const double v = (double)(lane * lane) - 100.5 * lane + 3.25;     // distinct, sign-changing values
    out[0 * 64 + lane] = wave_sum(v);
    out[1 * 64 + lane] = wave_max(v);
    out[2 * 64 + lane] = wave_min(v);
    out[3 * 64 + lane] = bcast(v, 37);
    out[4 * 64 + lane] = from_next_lane(v);
    out[5 * 64 + lane] = (double)__builtin_popcountll(ballot64(v > 0.0));
    out[6 * 64 + lane] = (double)bcast_i(lane * 3, 21);
    out[7 * 64 + lane] = v;
    double q4[4] = {v, v * v, 1.0 / (1.0 + lane), (double)(lane & 7) - v};
    wave_sum4(q4, lane);
    out[8 * 64 + lane] = q4[0]; out[9 * 64 + lane] = q4[1]; out[10 * 64 + lane] = q4[2]; out[11 * 64 + lane] = q4[3];
}

}  // namespace

// one switch of the table into its field: v is what the environment holds for it, or null for its default
static void set_switch(amx_ctx *ctx, const amx_switch &w, const char *v)
{
    const bool given = v && *v;
    long long c[3] = {w.dflt[0], w.dflt[1], w.dflt[2]};
    switch (w.kind) {
    case SW_FLAG: ctx->*w.flag = given && *v != '0'; break;
    case SW_OFF: ctx->*w.flag = v && *v == '0'; break;
    case SW_GIVEN: ctx->*w.flag = v != nullptr; break;
    case SW_CHAR: ctx->*w.num = v ? (unsigned char)*v : w.dflt[0]; break;
    case SW_INT: ctx->*w.num = given ? w.fix(atoll(v), w.dflt[0]) : w.dflt[0]; break;
    case SW_LIST:
        if (given) sscanf(v, w.fmt, &c[0], &c[1], &c[2]);
        for (int k = 0; k < 3; k++) (ctx->*w.list)[k] = given ? w.fix(c[k], w.dflt[k]) : c[k];
        break;
    }
}

// =================================================================== C ABI
extern "C" {

int amx_version(void) { return 100; }

int amx_device_count(void)
{
    int ndev = 0, n = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    for (int d = 0; d < ndev; d++) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) n = d + 1;     // (device numbers are HIP's)
    }
    return n;
}

int amx_ctx_create(int device, amx_ctx **out)
{
    if (!out) return AMX_E_BADARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return AMX_E_NODEVICE;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return AMX_E_NODEVICE; }
    if (device >= ndev) return AMX_E_NODEVICE;
    if (hipSetDevice(device) != hipSuccess) return AMX_E_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return AMX_E_NODEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return AMX_E_NODEVICE;   // code objects are gfx950 only
    amx_ctx *ctx = new amx_ctx();
    ctx->device = device;
    ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipMalloc((void **)&ctx->status_d, ST_WORDS * sizeof(int)) != hipSuccess ||
        hipHostMalloc((void **)&ctx->status_h, (ST_WORDS + 16) * sizeof(int), hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {   // (k_status_home writes it from the device)
        delete ctx;
        return AMX_E_HIP;
    }
    for (int k = 0; k < kEv; k++) { hipEventCreate(&ctx->ev[k]); ctx->ev_valid[k] = false; }
    for (const amx_switch &w : kSwitches) set_switch(ctx, w, getenv(w.name));      // the ONE place that reads the environment (amx_host.hpp)
    reset_status(ctx, nullptr);
    hipStreamSynchronize(nullptr);
    *out = ctx;
    return AMX_OK;
}

void amx_ctx_destroy(amx_ctx *ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    auto release = [](DevBuf &b) { if (b.p) hipFree(b.p); };
    ctx->for_each(release);
    ctx->alt.for_each(release);
    for (DevBuf *b : {&ctx->big, &ctx->hy, &ctx->hdirs, &ctx->hest, &ctx->hrmse, &ctx->hnrmse, &ctx->hextra, &ctx->hy32, &ctx->wy, &ctx->pred_idx, &ctx->debias_sigma, &ctx->debias_b0, &ctx->median_ws, &ctx->unring_ws}) release(*b);
    if (ctx->debias_stats) hipFree(ctx->debias_stats);
    if (ctx->debias_ev) (void)hipEventDestroy(ctx->debias_ev);
    if (ctx->san_count) hipFree(ctx->san_count);
    if (ctx->san_host) hipHostFree(ctx->san_host);
    for (hipEvent_t e : ctx->san_ev) if (e) (void)hipEventDestroy(e);
    if (ctx->status_d) hipFree(ctx->status_d);
    if (ctx->status_h) hipHostFree(ctx->status_h);
    for (int k = 0; k < kEv; k++) (void)hipEventDestroy(ctx->ev[k]);
    if (ctx->up_ev) (void)hipEventDestroy(ctx->up_ev);
    if (ctx->hs) { (void)hipStreamDestroy(ctx->hs); (void)hipStreamDestroy(ctx->hs2); for (hipEvent_t e : ctx->hev) (void)hipEventDestroy(e); }
    if (ctx->stage_thread.joinable()) ctx->stage_thread.join();
    delete ctx->stage_bg;
    for (int w = 0; w < 2; w++) if (ctx->fork_s[w]) { (void)hipStreamDestroy(ctx->fork_s[w]); for (hipEvent_t e : ctx->fork_ev[w]) if (e) (void)hipEventDestroy(e); }
    delete ctx->stage;             // (joins the host threads of the float32 transport)
    delete ctx;
}

const char *amx_last_error(amx_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

// status words home (the pinned mirror, written from the device) and cleared for the next call: one launch where a copy and two
// memsets were three nodes of the stream (~11 us each at the end of every call)
__global__ void k_status_home(int *__restrict__ st, int *__restrict__ home)
{
    const int i = threadIdx.x;
    if (i < ST_WORDS) {
        home[i] = st[i];
        st[i] = (i == ST_ERRPACK || i == ST_ERRPACK + 1) ? 0x7f7f7f7f : 0;
    }
    __threadfence_system();
}

int amx_sync_status(amx_ctx *ctx, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    static_assert(ST_WORDS <= 128, "k_status_home: one thread per status word");
    hipLaunchKernelGGL(k_status_home, dim3(1), dim3(128), 0, s, ctx->status_d, ctx->status_h);
#ifdef AMX_PHASES
    unsigned long long ph_[16];
    if (ctx->misc.p) HIPCHK(ctx, hipMemcpyAsync(ph_, (int *)ctx->misc.p + 16, sizeof ph_, hipMemcpyDeviceToHost, s));
#endif
    int rc = AMX_OK;
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(s));
#ifdef AMX_PHASES
    if (ctx->misc.p) {
        static const char *nm[8] = {"decode", "columns+gram", "cholesky", "solve+residual", "refinement", "norms", "screening", "exact-dots"};   // certified voxels: phases of certify_seed
        for (int st_ = 0; st_ < 2; st_++) {
            unsigned long long tot = 0;
            for (int k = 0; k < 8; k++) tot += ph_[st_ * 8 + k];
            fprintf(stderr, "[amx] NNLS stage %d phases:", st_ == 0 ? 1 : 3);
            for (int k = 0; k < 8; k++) fprintf(stderr, " %s %.1f%%", nm[k], tot ? 100.0 * ph_[st_ * 8 + k] / tot : 0.0);
            fprintf(stderr, "\n");
        }
    }
#endif
    const int *st = ctx->status_h;
    ctx->stats[0] = st[ST_RERUN];
    ctx->stats[1] = st[ST_ITCAP];
    ctx->stats[2] = st[ST_OVERFLOW];
    ctx->stats[3] = ((int64_t)st[ST_GUARD] << 32) | (unsigned)st[ST_GUARDVOX];
    ctx->seed_stats[0] = ctx->seeded_vox; ctx->seeded_vox = 0;
    for (int k = 0; k < 3; k++) { ctx->seed_stats[1 + k] = st[ST_LEFT + k] + ctx->uncert_vox[k]; ctx->uncert_vox[k] = 0; }
    ctx->seed_stats[4] = st[ST_CLIP];
    ctx->dense_stats[0] = st[ST_DENSE]; ctx->dense_stats[1] = st[ST_DENSE + 1];
    if (ctx->opt_debug) fprintf(stderr, "[amx] dual-vector evaluations per stage: exact %d %d %d  gram %d %d %d  inner iterations %d %d %d\n", st[ST_EXACT], st[ST_EXACT + 1], st[ST_EXACT + 2], st[ST_GRAM], st[ST_GRAM + 1], st[ST_GRAM + 2], st[ST_ITERS], st[ST_ITERS + 1], st[ST_ITERS + 2]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] seeds: stage 1 tried %d certified %d, stage 3 tried %d certified %d; seed solver trips %d lane-trips used %d; stage-1 refusals: malformed %d pivot %d refinement %d x<=0 %d dual %d\n", st[ST_SEED], st[ST_SEED + 1], st[ST_SEED + 2], st[ST_SEED + 3], st[ST_SEED + 4], st[ST_SEED + 5], st[ST_SEED + 7], st[ST_SEED + 8], st[ST_SEED + 9], st[ST_SEED + 10], st[ST_SEED + 11]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] screened certificates: %d exact dot products (NNLS stages), %d (LASSO stage)\n", st[ST_SEED + 22], st[ST_SEED + 23]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] Gram certificates stage 1: %d voxels, %d certified (pivot ratio %d, x <= 0 %d, dual %d), %d dual values; stage 3: %d voxels, %d certified (pivot %d, x <= 0 %d, dual %d), %d dual values\n",
                             st[ST_SEED + 24], st[ST_SEED + 25], st[ST_SEED + 26], st[ST_SEED + 27], st[ST_SEED + 28], st[ST_SEED + 29], st[ST_SEED + 30], st[ST_SEED + 31], st[ST_SEED + 32], st[ST_SEED + 33], st[ST_SEED + 34], st[ST_SEED + 35]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] Gram certificates LASSO: %d voxels, %d certified (more than 12 atoms %d, x <= 0 %d, dual %d), %d dual values\n",
                             st[ST_SEED + 36], st[ST_SEED + 37], st[ST_SEED + 38], st[ST_SEED + 39], st[ST_SEED + 40], st[ST_SEED + 41]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] Gram certificates LASSO, second pass: %d voxels, %d certified (more than 18 atoms %d, x <= 0 %d, dual %d), %d dual values\n",
                             st[ST_SEED + 48], st[ST_SEED + 49], st[ST_SEED + 50], st[ST_SEED + 51], st[ST_SEED + 52], st[ST_SEED + 53]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] LASSO seeds: tried %d certified %d; seed solver trips %d lane-trips used %d\n", st[ST_SEED + 18], st[ST_SEED + 19], st[ST_SEED + 20], st[ST_SEED + 21]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] LASSO seed solver kcycles (wave sums / 1024): take %d scan %d changes %d factor+solve %d; change() calls %d (one loop over the lanes' own lists: %d)\n", st[ST_SEED + 42], st[ST_SEED + 43], st[ST_SEED + 45], st[ST_SEED + 46], st[ST_SEED + 44], st[ST_SEED + 47]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] seed solver kcycles (wave sums / 1024): take %d solve+drop %d residual %d scan %d append %d store %d\n", st[ST_SEED + 12], st[ST_SEED + 13], st[ST_SEED + 14], st[ST_SEED + 15], st[ST_SEED + 16], st[ST_SEED + 17]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] Gram certificate kcycles (decode | gather+factor+solve | screening | exact duals | output): stage 1 %d %d %d %d %d, stage 3 %d %d %d %d %d\n",
                             st[ST_SEED + 60], st[ST_SEED + 61], st[ST_SEED + 62], st[ST_SEED + 63], st[ST_SEED + 64], st[ST_SEED + 65], st[ST_SEED + 66], st[ST_SEED + 67], st[ST_SEED + 68], st[ST_SEED + 69]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] LASSO Gram certificate kcycles (decode | gather+factor+solve | screening | exact duals | output): %d %d %d %d %d\n",
                             st[ST_SEED + 70], st[ST_SEED + 71], st[ST_SEED + 72], st[ST_SEED + 73], st[ST_SEED + 74]);
    if (ctx->opt_debug) fprintf(stderr, "[amx] stage-3 seed solver kcycles: take %d solve+drop %d residual %d scan %d append %d store %d\n", st[ST_SEED + 54], st[ST_SEED + 55], st[ST_SEED + 56], st[ST_SEED + 57], st[ST_SEED + 58], st[ST_SEED + 59]);
    if (ctx->opt_debug && st[ST_GRAM + 1] > 0) fprintf(stderr, "[amx] k_noddi_lasso_big: %d voxels, %.1f pivoting steps per voxel\n", st[ST_GRAM + 1], (double)st[ST_ITERS + 1] / st[ST_GRAM + 1]);
    {
        // first offending voxel and what it held, as the kernels' one 64-bit atomicMin left them
        int *sth = ctx->status_h;
        const unsigned lo = (unsigned)sth[ST_ERRPACK], hi = (unsigned)sth[ST_ERRPACK + 1];
        sth[ST_ERRVOX] = (int)hi;
        if (hi != 0x7f7f7f7fu) {
            if (sth[ST_ERRKIND] == 1) sth[ST_II1] = (int)lo;                                   // (ST_II2 = number of dictionaries, stored by the kernel)
            else { sth[ST_II1] = (int)(lo >> 16) - 1; sth[ST_II2] = (int)(lo & 0xffffu) - 1; }
        }
    }
    if (st[ST_ERRVOX] != 0x7f7f7f7f) {
        char b[256];
        snprintf(b, sizeof b, "\"amico.lut.dir_to_lut_idx\" index out of bounds (%d, %d) [voxel %d]", st[ST_II1], st[ST_II2], st[ST_ERRVOX]);
        ctx->err = b;
        return AMX_E_DIR_OOB;
    }
    if (st[ST_OVERFLOW] > 0) {
        char b[256];
        snprintf(b, sizeof b, "%d voxel(s) exceeded the largest supported active set", st[ST_OVERFLOW]);
        ctx->err = b;
        return AMX_E_OVERFLOW;
    }
    return AMX_OK;
}

int amx_set_progress(amx_ctx *ctx, void (*callback)(int64_t done, int64_t total, void *user), void *user)
{
    if (!ctx) return AMX_E_BADARG;
    ctx->progress = callback;
    ctx->progress_user = user;
    return AMX_OK;
}

// diagnosis / tests: copy a workspace buffer of the LAST fit (which 0 .. 7), a table of the dictionary `lut` (10 .. 33) or the Gram
// tables of a dense amx_dict (40, the handle in lut's place) to the host.  The codes, their layouts and shapes: include/amico_amd.h.
// Every copy is checked against the table's own size; a table that was never built or belongs to another model is refused.
int amx_debug_fetch(amx_ctx *ctx, const amx_lut *lut, int which, void *dst, size_t bytes)
{
    if (!ctx || !dst) return AMX_E_BADARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    const void *src = nullptr;
    size_t have = 0;
    bool host = false;                 // (a value kept in the handle itself)
    int s2d = 0;
    if (which >= 0 && which <= 7) {
        const DevBuf *b = nullptr;
        switch (which) {
        case 0: b = &ctx->perm; break;
        case 1: b = &ctx->ytil; break;
        case 2: b = &ctx->seeds; break;
        case 3: b = &ctx->ytil2; break;
        case 4: b = &ctx->seeds2; break;
        case 5: b = &ctx->cgemm; break;
        case 6: b = &ctx->schunks; break;
        default: b = &ctx->misc; break;
        }
        src = b->p; have = b->cap;
        if (!src) return amx_bad(ctx, "amx_debug_fetch: no fit on this context has made that workspace buffer");
    } else if (which == 40) {
        const amx_dict *dict = reinterpret_cast<const amx_dict *>(lut);
        if (!dict || dict->model != kDictModel) return amx_bad(ctx, "amx_debug_fetch: which = 40 reads an amx_dict handle");
        if (dict->ctx != ctx) return amx_bad(ctx, "amx_debug_fetch: the dictionary belongs to another context");
        if (!dict->dense || !dict->gram) return amx_bad(ctx, "amx_debug_fetch: the dictionary is not dense (amx_dict_set_dense): it has no Gram tables");
        src = dict->gram; have = (size_t)dict->n_dicts * dict->n * dict->ldG * sizeof(double);
    } else if (which >= 10 && which <= 33) {
        if (!lut) return amx_bad(ctx, "amx_debug_fetch: this table needs a dictionary handle");
        if (lut->model < 1 || lut->model > 4) return amx_bad(ctx, "amx_debug_fetch: not an amx_lut handle");
        if (lut->ctx != ctx) return amx_bad(ctx, "amx_debug_fetch: the dictionary belongs to another context");
        const bool noddi = lut->model == 1;
        const size_t nd = (size_t)lut->ndirs, f64 = sizeof(double);
        int want_model = 1;            // 0: any
        switch (which) {
        case 10: src = lut->basis_U; have = nd * lut->nS * kSeedKD * f64; break;
        case 11: src = lut->basis_S; have = nd * lut->n_atoms * kSeedKD * f64; break;
        case 12: src = lut->basis2_U; have = nd * lut->nS * kSeedKD * f64; break;
        case 13: src = lut->basis2_S; have = nd * lut->n_wm * kSeedKD * f64; break;
        case 14: want_model = 0; src = lut->tiles; have = nd * lut->tile_stride * (lut->model == 3 ? f64 : sizeof(float)); break;
        case 15: want_model = 0; src = lut->gram; have = nd * lut->n_atoms * lut->ldG * f64; break;
        case 16: src = lut->gram_dwi; have = nd * lut->n_atoms * lut->ldG * f64; break;
        case 17: src = lut->screen_S; have = nd * kSeedKD * kScreenLd * sizeof(float); break;
        case 18: src = lut->screen2_S; have = nd * kSeedKD * kScreenLd * sizeof(float); break;
        case 19: src = lut->screen_kappa; have = nd * f64; break;
        case 20: src = lut->screen_kappa0; have = nd * f64; break;
        case 21: src = lut->screen2_kappa; have = nd * f64; break;
        case 22: src = lut->screen2_kappa0; have = nd * f64; break;
        case 23: src = lut->u2iso; have = nd * kSeedKD * f64; break;
        case 24: src = lut->rowdwi; have = (size_t)lut->nS; break;
        case 25: src = lut->colscale; have = (size_t)lut->n_atoms * f64; break;
        case 26: host = true; s2d = lut->s2_derive; src = &s2d; have = sizeof(int); break;
        case 30: want_model = 2; src = lut->fw_prep; have = src ? nd * amx_fw_table_words(lut) * f64 : 0; break;
        case 31: want_model = 4; src = lut->czb_prep; have = nd * amx_czb_table_stride(lut->nS) * f64; break;
        case 32: want_model = 3; src = lut->sandi_prep; have = amx_sandi_table_words() * f64; break;
        case 33: want_model = 3; src = lut->sandi_long_prep; have = amx_sandi_long_table_words(lut) * f64; break;
        default: return amx_bad(ctx, "amx_debug_fetch: no such table");
        }
        if (want_model && lut->model != want_model) return amx_bad(ctx, "amx_debug_fetch: the dictionary's model has no such table");
        if (!src) return amx_bad(ctx, (which >= 30) ? "amx_debug_fetch: no fit has built that table yet (it is made for one lambda2 by the first fit that reads it)"
                                      : (noddi && which != 15 && which != 14) ? "amx_debug_fetch: the dictionary has no such table (no seeds for more than 160 atoms)"
                                                                               : "amx_debug_fetch: the dictionary has no such table");
    } else return amx_bad(ctx, "amx_debug_fetch: no such buffer");
    if (bytes > have) {
        char b[160];
        snprintf(b, sizeof b, "amx_debug_fetch: %zu bytes asked of a table of %zu (which = %d)", bytes, have, which);
        return amx_bad(ctx, b);
    }
    if (host) memcpy(dst, src, bytes);
    else HIPCHK(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return AMX_OK;
}

int amx_set_debug_x(amx_ctx *ctx, double *d_x)
{
    if (!ctx) return AMX_E_BADARG;
    ctx->dbg_x = d_x;
    return AMX_OK;
}

int amx_set_fw_iso(amx_ctx *ctx, double *d_xiso)
{
    if (!ctx) return AMX_E_BADARG;
    ctx->fw_iso = d_xiso;
    return AMX_OK;
}

int amx_selftest(amx_ctx *ctx, double *out512)
{
    if (!ctx || !out512) return AMX_E_BADARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = amx_ensure(ctx, ctx->hest, 768 * sizeof(double)))) return rc;
    hipLaunchKernelGGL(k_selftest, dim3(1), dim3(64), 0, nullptr, (double *)ctx->hest.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpy(out512, ctx->hest.p, 768 * sizeof(double), hipMemcpyDeviceToHost));
    return AMX_OK;
}

int amx_set_profiling(amx_ctx *ctx, int enable)
{
    if (!ctx) return AMX_E_BADARG;
    ctx->profiling = (enable >= 0 && enable <= 11) ? enable : 1;
    for (int k = 0; k < kEv; k++) ctx->ev_valid[k] = false;
    return AMX_OK;
}

int amx_last_kernel_ms(amx_ctx *ctx, int which, float *out_ms)
{
    if (!ctx || !out_ms || which < 0 || which > 9) return AMX_E_BADARG;
    const int a = which == 0 ? 0 : 2 * which, b = which == 0 ? 1 : 2 * which + 1;
    if (!ctx->ev_valid[a] || !ctx->ev_valid[b]) return amx_bad(ctx, "amx_last_kernel_ms: no profiled call");
    HIPCHK(ctx, hipEventSynchronize(ctx->ev[b]));
    HIPCHK(ctx, hipEventElapsedTime(out_ms, ctx->ev[a], ctx->ev[b]));
    return AMX_OK;
}

int amx_last_stats(amx_ctx *ctx, int64_t out[4])
{
    if (!ctx || !out) return AMX_E_BADARG;
    for (int k = 0; k < 4; k++) out[k] = ctx->stats[k];
    return AMX_OK;
}

int amx_last_host_narrowed(amx_ctx *ctx) { return ctx ? ctx->host_narrowed : 0; }

int amx_set_call_voxels(amx_ctx *ctx, int64_t total)
{
    if (!ctx || total < 0) return AMX_E_BADARG;
    ctx->call_total_vox = total;
    return AMX_OK;
}

int amx_host_pool_info(amx_ctx *ctx, int out[4])
{
    if (!ctx || !out) return AMX_E_BADARG;
    out[0] = ctx->stage ? ctx->stage->threads() : 0;
    out[1] = ctx->stage ? ctx->stage->share_first() : -1;
    out[2] = ctx->stage ? ctx->stage->share_cores() : 0;
    out[3] = ctx->device;
    return AMX_OK;
}

int amx_last_path(amx_ctx *ctx, char *buf, int cap)
{
    if (!ctx || !buf || cap <= 0) return AMX_E_BADARG;
    snprintf(buf, (size_t)cap, "%s", ctx->path.c_str());
    return AMX_OK;
}

// the route of a NODDI fit (amx_noddi_route.hpp) for a dictionary of this shape, as amx_lut_upload_noddi would build it, with every switch at its default
int amx_noddi_route(int nS, int n_wm, int n_dwi, int ndirs, int is_exvivo, int64_t n_vox, int64_t call_vox, double lambda1, double lambda2,
                    char *path, int cap, int64_t out[AMX_ROUTE_WORDS])
{
    if (!path || cap <= 0 || !out || nS < 1 || nS > 512 || n_wm < 1 || n_wm + 1 + (is_exvivo ? 1 : 0) > 256 || n_dwi < 0 || n_dwi > nS || ndirs < 1 ||
        n_vox < 1 || call_vox < 0 || !(lambda1 >= 0.0) || !(lambda2 >= 0.0)) return AMX_E_BADARG;
    amx_ctx defaults;      // (holds the switches only: nothing in here touches the device)
    for (const amx_switch &w : kSwitches) set_switch(&defaults, w, nullptr);      // (no environment here: every switch at the table's default)
    const int n_atoms = n_wm + 1 + (is_exvivo ? 1 : 0);
    const amx::NoddiShape sh{nS, (n_atoms & 1) ? n_atoms : n_atoms + 1, n_atoms, n_wm, n_dwi, ndirs, is_exvivo ? 1 : 0, is_exvivo ? 0 : 1, amx::noddi_tables(n_atoms, n_wm)};
    const amx::NoddiRoute r = amx::noddi_route(sh, {n_vox, call_vox > n_vox ? call_vox : n_vox, lambda1, lambda2}, noddi_switches(&defaults));
    const int64_t words[] = {r.seeds, r.global, r.gemm_ks, r.gemm_n_pass, r.gemm_win, r.gcert, r.repair, r.rescue, r.tile_in_lds, r.seeds2, r.gcert2, r.wide, r.third,
                             r.min_items, r.seed2_max_atoms, r.seed2_trip_add, r.left2_second_half, r.left2_count, r.seed_occ2, r.seed2_occ2, r.seed_chunk,
                             r.seed_waves, r.seed1_waves, r.seed2_waves, r.s1.build, r.s2.build, r.s2.gram, r.s3.build, r.n_launch, r.gemm, r.NR, (int64_t)r.gcert2_wide_lds};
    static_assert(sizeof words / sizeof words[0] + 3 * (sizeof r.launch / sizeof r.launch[0]) <= AMX_ROUTE_WORDS, "amx_noddi_route: out[] too short");
    int k = 0;
    for (int64_t w : words) out[k++] = w;
    std::string p;
    for (int l = 0; l < r.n_launch; l++) {
        p += (l ? " -> " : ""); p += r.launch[l].note;
        out[k++] = r.launch[l].waves; out[k++] = (int64_t)r.launch[l].lds; out[k++] = (int64_t)r.launch[l].lds_list;
    }
    snprintf(path, (size_t)cap, "%s", p.c_str());
    return AMX_OK;
}

// the route of a FreeWater, SANDI or CylinderZeppelinBall fit (amx_small_route.hpp) for a dictionary of this shape, as the model's upload would build it
int amx_small_route(int model, int nS, int n_atoms, int ndirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, int f32,
                    unsigned switches_mask, char *note_buf, int cap, int64_t out[AMX_SMALL_ROUTE_WORDS])
{
    if (!note_buf || cap <= 0 || !out || model < 2 || model > 4 || nS < 1 || nS > 512 || n_atoms < 1 || n_atoms > amx::kBigMaxAtoms || ndirs < 1 ||
        (model == 3 && ndirs != 1) || n_vox < 1 || n_vox > INT_MAX / 4 || !(lambda1 >= 0.0) || !(lambda2 >= 0.0) || switches_mask > 15u) return AMX_E_BADARG;
    // (ldA: new_lut's; Gram tables: amx_lut_upload_czb's, and amx_build_big_gram for every dictionary of more than 64 atoms)
    const amx::SmallShape sh{model, nS, (n_atoms & 1) ? n_atoms : n_atoms + 1, n_atoms, ndirs, model == 4 || n_atoms > amx::kSmallMaxAtoms};
    const amx::SmallRoute r = amx::small_route(sh, {n_vox, lambda1, lambda2, flags, f32 != 0},
                                               {(switches_mask & 1u) != 0, (switches_mask & 2u) != 0, (switches_mask & 4u) != 0, (switches_mask & 8u) != 0});
    const int64_t words[AMX_SMALL_ROUTE_WORDS] = {r.family, r.N, r.NR, r.mfma, r.widen, r.chunk, r.blocks_chunk, r.tables, r.in_order, r.nSp, r.waves,
                                                  (int64_t)r.lds, (int64_t)r.lds_list, r.refusal, r.n_launch};
    for (int k = 0; k < AMX_SMALL_ROUTE_WORDS; k++) out[k] = words[k];
    std::string p;
    for (int l = 0; l < r.n_launch; l++) { p += (l ? " -> " : ""); p += r.launch[l]; }
    if (r.refusal) { p += "\n"; p += r.error; }
    snprintf(note_buf, (size_t)cap, "%s", p.c_str());
    return AMX_OK;
}

int amx_last_seed_stats(amx_ctx *ctx, int64_t out[8])
{
    if (!ctx || !out) return AMX_E_BADARG;
    for (int k = 0; k < 8; k++) out[k] = ctx->seed_stats[k];
    return AMX_OK;
}

}  // extern "C"

#ifdef AMX_PEEK
// diagnosis only (never built into the shipped library): read back the stage intermediates of one voxel
extern "C" int amx_peek(amx_ctx *ctx, int64_t vox, double *xiso2, unsigned long long *supp4)
{
    HIPCHK(ctx, hipMemcpy(xiso2, (double *)ctx->xiso.p + vox * 2, 2 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(supp4, (unsigned long long *)ctx->supp.p + vox * 4, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return AMX_OK;
}
#endif
