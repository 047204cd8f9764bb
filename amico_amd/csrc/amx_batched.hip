// amx_batched.hip -- the solvers the reference binds (cyspams.interfaces.nnls / lasso, models.pyx:18), batched over voxels
#include "amx_launch.hpp"
using namespace amx;

// dense: the dictionary keeps its Gram tables (amx_dict_set_dense) -- what overflows the re-run pass goes to list 6 and k_batched_big takes it
template <int NR, bool RIDGE>
static int go(amx_ctx *ctx, BatchedArgs &a, const Plan &pl, hipStream_t s, bool dense)
{
    constexpr int NQ = 3, MP = 16, MB = 48;      // passive set of the main pass / of the one-wavefront re-run pass (48: its triangular factors still fit next to a 99 x 145 fp64 tile)
    constexpr int NW = 8;
    return launch_pair<NW>(ctx, a, pl, s, k_batched<NR, NQ, MP, NW, RIDGE, false>, k_batched<NR, NQ, MB, 1, RIDGE, true>,
                           [&](int nw) { return fit_lds_bytes<double>(a.c.nS, a.c.ldA, NR, NQ, nw, MP, false, RIDGE); },
                           fit_lds_bytes<double>(a.c.nS, a.c.ldA, NR, NQ, 1, MB, false, RIDGE), 0, 2, "wavefront-per-voxel solver", dense);
}

// dictionaries beyond the LDS variants (m > 256 samples, n > 192 atoms, or an fp64 tile larger than a CU's LDS): the same solver with
// the tile read where it lies (k_batched<..., GT = true>: 8 rows / 4 atoms per lane: m <= 512, n <= 256)
template <bool RIDGE>
static int go_global(amx_ctx *ctx, BatchedArgs &a, const Plan &pl, hipStream_t s, bool dense)
{
    constexpr int NR = 8, NQ = 4, MP = 16, MB = 48, NW = 4;
    return launch_pair<NW>(ctx, a, pl, s, k_batched<NR, NQ, MP, NW, RIDGE, false, true>, k_batched<NR, NQ, MB, 1, RIDGE, true, true>,
                           [&](int nw) { return fit_lds_bytes<double>(a.c.nS, a.c.ldA, NR, NQ, nw, MP, false, RIDGE, true); },
                           fit_lds_bytes<double>(a.c.nS, a.c.ldA, NR, NQ, 1, MB, false, RIDGE, true), 0, 2, "wavefront-per-voxel solver", dense);
}

bool amx_batched_tile_global(int m, int ldA, int n)
{
    if (m > 256 || n > 192) return true;
    return fit_lds_bytes<double>(m, ldA, m <= 128 ? 2 : 4, 3, 1, 48, false, true) > kLdsPerCU;
}

int amx_launch_batched(amx_ctx *ctx, BatchedArgs &a, const Plan &pl, hipStream_t s, bool ridge, bool dense)
{
    if (amx_batched_tile_global(a.c.nS, a.c.ldA, a.c.n_atoms)) return ridge ? go_global<true>(ctx, a, pl, s, dense) : go_global<false>(ctx, a, pl, s, dense);
    if (ridge) return a.c.nS <= 128 ? go<2, true>(ctx, a, pl, s, dense) : go<4, true>(ctx, a, pl, s, dense);
    return a.c.nS <= 128 ? go<2, false>(ctx, a, pl, s, dense) : go<4, false>(ctx, a, pl, s, dense);
}

// ------------------------------------------------------------------ the C entry points
static int batched_dev(amx_ctx *ctx, const amx_dict *dict, const int32_t *d_idx, const double *d_y, int64_t n_vox, double lambda1, double lambda2,
                       bool ridge, double *d_x, double *d_rnorm, void *hip_stream)
{
    if (!ctx) return AMX_E_BADARG;
    if (!dict || dict->ctx != ctx) return amx_bad(ctx, "amx_*_batched: not a dictionary of this ctx");
    if (n_vox < 0 || n_vox > INT_MAX / 4) return amx_bad(ctx, "amx_*_batched: bad n_vox");
    if (n_vox == 0) return AMX_OK;
    if (!d_y || !d_x) return amx_bad(ctx, "amx_*_batched: null buffer");
    if (ridge && (!(lambda1 >= 0.0) || !(lambda2 >= 0.0))) return amx_bad(ctx, "amx_lasso_batched: need lambda1 >= 0 and lambda2 >= 0");
    if (!d_idx && dict->n_dicts != 1) return amx_bad(ctx, "amx_*_batched: dict_idx may only be NULL for a single dictionary");
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Plan pl; int rc;
    if ((rc = make_plan(ctx, n_vox, dict->n_dicts, pl))) return rc;
    clear_events(ctx);
    rec(ctx, 0, s);
    if ((rc = enqueue_index_bucketing(ctx, d_idx, dict->n_dicts, n_vox, pl, s))) return rc;
    BatchedArgs a;
    memset(&a, 0, sizeof a);
    fill_common(a.c, dict->tiles, d_y, nullptr, pl, ctx->status_d, dict->m, dict->ldA, dict->n, dict->tile_stride, lambda1, lambda2, 0);
    a.x = d_x; a.rnorm = d_rnorm;
    // (voxels with a bad dictionary index are skipped: defined zeros)
    HIPCHK(ctx, hipMemsetAsync(d_x, 0, (size_t)n_vox * dict->n * sizeof(double), s));
    rc = amx_launch_batched(ctx, a, pl, s, ridge, dict->dense);
    if (!rc && dict->dense) rc = amx_launch_batched_big(ctx, a, dict, pl, s);      // (one launch that finds a zero count when nothing overflowed)
    fold_counters(ctx, s);
    rec(ctx, 1, s);
    return rc;
}

extern "C" {

int amx_dict_upload(amx_ctx *ctx, const double *A, int m, int n, int n_dicts, amx_dict **out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!A || !out || m <= 0 || n <= 0 || n_dicts <= 0) return amx_bad(ctx, "amx_dict_upload: bad argument");
    // (dictionaries that fit a CU's LDS as fp64 are staged there; larger ones -- up to 512 samples x 256 atoms, what a wavefront's lanes
    //  hold -- are read where they lie: amx_batched.hip)
    if (n > 256 || m > 512) return amx_bad(ctx, "amx_dict_upload: unsupported size (n <= 256 atoms, m <= 512 samples)");
    const int ldA = (n & 1) ? n : n + 1;
    const int tile_stride = (m * ldA + 3) & ~3;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> t((size_t)n_dicts * tile_stride + kTileSlack, 0.0);
    for (int d = 0; d < n_dicts; d++)
        for (int j = 0; j < n; j++)
            for (int i = 0; i < m; i++) t[(size_t)d * tile_stride + (size_t)i * ldA + j] = A[((size_t)d * n + j) * m + i];     // column-major in, ld = m
    amx_dict *h = new amx_dict();
    h->ctx = ctx; h->m = m; h->n = n; h->ldA = ldA; h->tile_stride = tile_stride; h->n_dicts = n_dicts;
    int rc;
    if ((rc = amx_upload(ctx, &h->tiles, t.data(), t.size()))) { delete h; return rc; }
    *out = h;
    return AMX_OK;
}

void amx_dict_destroy(amx_dict *h)
{
    if (!h) return;
    if (h->ctx) hipSetDevice(h->ctx->device);
    if (h->tiles) hipFree(h->tiles);
    if (h->gram) hipFree(h->gram);
    delete h;
}

int amx_dict_set_dense(amx_ctx *ctx, amx_dict *dict, int on)
{
    if (!ctx) return AMX_E_BADARG;
    if (!dict || dict->ctx != ctx) return amx_bad(ctx, "amx_dict_set_dense: not a dictionary of this ctx");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!on) {
        dict->dense = false;
        if (dict->gram) HIPCHK(ctx, hipFree(dict->gram));              // (waits for the kernels that read it)
        dict->gram = nullptr;
        return AMX_OK;
    }
    if (dict->dense) return AMX_OK;
    const int ldG = dict->ldA;
    double *g = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&g, (size_t)dict->n_dicts * dict->n * ldG * sizeof(double)));      // (failure: the dictionary stays as it was)
    dict->gram = g; dict->ldG = ldG;
    const int rc = amx_build_dict_gram(ctx, dict);
    if (rc) { (void)hipFree(g); dict->gram = nullptr; return rc; }
    dict->dense = true;
    return AMX_OK;
}

int amx_batched_last_dense(amx_ctx *ctx, int64_t out[2])
{
    if (!ctx || !out) return AMX_E_BADARG;
    out[0] = ctx->dense_stats[0]; out[1] = ctx->dense_stats[1];
    return AMX_OK;
}

int amx_nnls_batched_device(amx_ctx *ctx, const amx_dict *dict, const int32_t *d_dict_idx, const double *d_y, int64_t n_vox, double *d_x,
                            double *d_rnorm, void *hip_stream)
{
    return batched_dev(ctx, dict, d_dict_idx, d_y, n_vox, 0.0, 0.0, false, d_x, d_rnorm, hip_stream);
}

int amx_lasso_batched_device(amx_ctx *ctx, const amx_dict *dict, const int32_t *d_dict_idx, const double *d_y, int64_t n_vox, double lambda1,
                             double lambda2, double *d_x, void *hip_stream)
{
    return batched_dev(ctx, dict, d_dict_idx, d_y, n_vox, lambda1, lambda2, true, d_x, nullptr, hip_stream);
}

static int batched_host(amx_ctx *ctx, const amx_dict *dict, const int32_t *idx, const double *y, int64_t n_vox, double lambda1, double lambda2, bool ridge,
                        double *x, double *rnorm)
{
    if (!ctx) return AMX_E_BADARG;
    const std::string who = ridge ? "amx_lasso_batched" : "amx_nnls_batched";
    if (!dict || dict->ctx != ctx) return amx_bad(ctx, (who + ": not a dictionary of this ctx").c_str());
    if (n_vox == 0) return AMX_OK;
    if (n_vox < 0 || n_vox > INT_MAX / 4) return amx_bad(ctx, (who + ": bad n_vox").c_str());      // (before anything is sized from it)
    if (!y || !x) return amx_bad(ctx, (who + ": null buffer").c_str());
    if (ridge && (!(lambda1 >= 0.0) || !(lambda2 >= 0.0))) return amx_bad(ctx, "amx_lasso_batched: need lambda1 >= 0 and lambda2 >= 0");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    AMX_H2D(ctx->hy, y, (size_t)n_vox * dict->m * sizeof(double))
    if (idx) { AMX_H2D(ctx->hdirs, idx, (size_t)n_vox * sizeof(int32_t)) }
    if ((rc = amx_ensure(ctx, ctx->hest, (size_t)n_vox * dict->n * sizeof(double)))) return rc;
    if (rnorm && (rc = amx_ensure(ctx, ctx->hrmse, (size_t)n_vox * sizeof(double)))) return rc;
    if ((rc = batched_dev(ctx, dict, idx ? (const int32_t *)ctx->hdirs.p : nullptr, (const double *)ctx->hy.p, n_vox, lambda1, lambda2, ridge,
                          (double *)ctx->hest.p, rnorm ? (double *)ctx->hrmse.p : nullptr, nullptr))) return rc;
    const int rcs = amx_sync_status(ctx, nullptr);
    if (rcs == AMX_E_DIR_OOB) {
        const int *st = ctx->status_h;
        char b[256];
        snprintf(b, sizeof b, "%s: dict_idx out of range (%d, dictionaries: %d) [voxel %d]", who.c_str(), st[ST_II1], st[ST_II2], st[ST_ERRVOX]);
        ctx->err = b;
    } else if (rcs) return rcs;
    // (a bad dict_idx: every other voxel is solved, the offending ones hold zeros -- the caller gets those results with the error code,
    //  as include/amico_amd.h says)
    HIPCHK(ctx, hipMemcpy(x, ctx->hest.p, (size_t)n_vox * dict->n * sizeof(double), hipMemcpyDeviceToHost));
    if (rnorm) HIPCHK(ctx, hipMemcpy(rnorm, ctx->hrmse.p, (size_t)n_vox * sizeof(double), hipMemcpyDeviceToHost));
    return rcs;
}

int amx_nnls_batched(amx_ctx *ctx, const amx_dict *dict, const int32_t *dict_idx, const double *y, int64_t n_vox, double *x, double *rnorm)
{
    return batched_host(ctx, dict, dict_idx, y, n_vox, 0.0, 0.0, false, x, rnorm);
}

int amx_lasso_batched(amx_ctx *ctx, const amx_dict *dict, const int32_t *dict_idx, const double *y, int64_t n_vox, double lambda1, double lambda2, double *x)
{
    return batched_host(ctx, dict, dict_idx, y, n_vox, lambda1, lambda2, true, x, nullptr);
}

}  // extern "C"
