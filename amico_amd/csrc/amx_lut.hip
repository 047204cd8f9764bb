// amx_lut.hip -- the dictionaries of the four models: upload, the tables made from them on the device, destroy.
#include "amx_host.hpp"
#include "amx_build.hpp"

using namespace amx;

// the dictionary every upload starts from; the host threads of the float32 transport are made beside the upload
static amx_lut *new_lut(amx_ctx *ctx, int model, int nS, int n_atoms, int ndirs)
{
    prefetch_stage_pool(ctx);
    amx_lut *lut = new amx_lut();
    lut->ctx = ctx; lut->model = model; lut->nS = nS; lut->n_atoms = n_atoms; lut->ndirs = ndirs;
    lut->ldA = (n_atoms & 1) ? n_atoms : n_atoms + 1;         // odd: conflict-free LDS columns
    lut->tile_stride = (nS * lut->ldA + 3) & ~3;
    return lut;
}

static int build_tiles(amx_ctx *ctx, amx_lut *lut, const float *src, size_t src_n, const float *fix,
                       size_t fix_n, const std::vector<int> &fix_ones, int n_lut)
{
    float *d_src = nullptr, *d_fix = nullptr; int *d_ones = nullptr;
    int rc;
    if ((rc = amx_upload(ctx, &d_src, src, src_n))) return rc;
    if ((rc = amx_upload(ctx, &d_fix, fix, fix_n ? fix_n : 1))) return rc;
    if ((rc = amx_upload(ctx, &d_ones, fix_ones.data(), fix_ones.size()))) return rc;
    const size_t bytes = ((size_t)lut->ndirs * lut->tile_stride + kTileSlack) * sizeof(float) + 64;   // (slack: the global-tile kernels' row sweeps read past the last row's end)
    HIPCHK(ctx, hipMalloc(&lut->tiles, bytes));
    HIPCHK(ctx, hipMemset(lut->tiles, 0, bytes));
    hipLaunchKernelGGL(k_build_lut, dim3(2048), dim3(256), 0, nullptr, d_src, d_fix, d_ones, n_lut,
                       (int)fix_ones.size(), lut->ndirs, lut->nS, lut->ldA, lut->tile_stride, (float *)lut->tiles);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipDeviceSynchronize());
    hipFree(d_src); hipFree(d_fix); hipFree(d_ones);
    return AMX_OK;
}

extern "C" {

void amx_lut_destroy(amx_lut *lut)
{
    if (!lut) return;
    if (lut->ctx) hipSetDevice(lut->ctx->device);
    void *ps[] = {lut->u2iso, lut->screen2_kappa0, lut->screen_kappa0, lut->screen2_S, lut->screen2_kappa, lut->screen_S, lut->screen_kappa, lut->basis_U, lut->basis_S, lut->basis2_U, lut->basis2_S, lut->gram, lut->gram_dwi, lut->tiles, lut->htable, lut->rowdwi, lut->colscale, lut->icvf, lut->kappa,
                  lut->norms, lut->Rs, lut->d_in, lut->d_isos, lut->fw_prep, lut->sandi_prep, lut->sandi_long_prep, lut->czb_prep};
    for (void *p : ps) if (p) hipFree(p);
    if (lut->fw_ready) (void)hipEventDestroy(lut->fw_ready);
    if (lut->sandi_ready) (void)hipEventDestroy(lut->sandi_ready);
    if (lut->sandi_long_ready) (void)hipEventDestroy(lut->sandi_long_ready);
    if (lut->czb_ready) (void)hipEventDestroy(lut->czb_ready);
    delete lut;
}

int amx_lut_upload_noddi(amx_ctx *ctx, const float *wm, const float *iso, const double *norms,
                         const float *icvf, const float *kappa, const int16_t *htable,
                         const int64_t *dwi_idx, int n_wm, int ndirs, int nS, int dwi_count,
                         int is_exvivo, amx_lut **out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!wm || !iso || !norms || !icvf || !kappa || !htable || !dwi_idx || !out || n_wm <= 0 || ndirs <= 0 ||
        nS <= 0 || dwi_count < 0 || dwi_count > nS)
        return amx_bad(ctx, "amx_lut_upload_noddi: bad argument");
    const int n_atoms = n_wm + 1 + (is_exvivo ? 1 : 0);
    // any shape models.pyx:825-861 would run, up to what a wavefront's lanes hold: 8 rows / 4 atoms per lane
    if (n_atoms > 256 || nS > 512) return amx_bad(ctx, "amx_lut_upload_noddi: unsupported size (n_atoms <= 256, nS <= 512)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    amx_lut *lut = new_lut(ctx, 1, nS, n_atoms, ndirs);
    lut->n_wm = n_wm; lut->is_exvivo = is_exvivo;
    int rc;
    std::vector<int> ones;
    std::vector<float> fix;
    if (is_exvivo) { ones.push_back(1); fix.insert(fix.end(), nS, 1.0f); }   // models.pyx:843-844
    ones.push_back(0); fix.insert(fix.end(), iso, iso + nS);
    if ((rc = build_tiles(ctx, lut, wm, (size_t)n_wm * ndirs * nS, fix.data(), fix.size(), ones, n_wm))) { amx_lut_destroy(lut); return rc; }
    // rows of stage 2 (models.pyx:820, 917-921): j+1 if nS == 1+dwi_count ("single_b0") else dwi_idx[j]
    std::vector<unsigned char> rowdwi(nS, 0);
    const bool single_b0 = (nS == 1 + dwi_count);
    for (int j = 0; j < dwi_count; j++) {
        const int64_t row = single_b0 ? j + 1 : dwi_idx[j];
        if (row < 0 || row >= nS) { amx_lut_destroy(lut); return amx_bad(ctx, "amx_lut_upload_noddi: dwi_idx out of range"); }
        rowdwi[row] = 1;
    }
    // Are the rows outside stage 2 (the b0 volumes) exactly 1.0 in every atom, as resample_kernel leaves them (lut.pyx:298, 305)?
    // Then the stage-2 products of an unclipped voxel derive from the stage-1 table (k_noddi_gemm); otherwise every voxel takes
    // the exact pass.
    lut->n_dwi = dwi_count;
    lut->s2_derive = is_exvivo ? 0 : 1;
    for (int i = 0; i < nS && lut->s2_derive; i++) {
        if (rowdwi[i]) { if (!(iso[i] > 1e-30f) || !(iso[i] <= 3.0e38f)) lut->s2_derive = 0; continue; }
        if (iso[i] != 1.0f) lut->s2_derive = 0;
        for (size_t kd = 0; kd < (size_t)n_wm * ndirs && lut->s2_derive; kd++) if (wm[kd * nS + i] != 1.0f) lut->s2_derive = 0;
    }
    std::vector<double> colscale(n_atoms, 1.0);
    for (int k = 0; k < n_wm; k++) colscale[k] = dwi_count > 0 ? norms[k] : 1.0;   // rows of norms are identical
    std::vector<short> ht(htable, htable + 181 * 181);
    if ((rc = amx_upload(ctx, &lut->rowdwi, rowdwi.data(), rowdwi.size())) ||
        (rc = amx_upload(ctx, &lut->colscale, colscale.data(), colscale.size())) ||
        (rc = amx_upload(ctx, &lut->icvf, icvf, (size_t)n_wm)) || (rc = amx_upload(ctx, &lut->kappa, kappa, (size_t)n_wm)) ||
        (rc = amx_upload(ctx, &lut->htable, ht.data(), ht.size()))) { amx_lut_destroy(lut); return rc; }
    // Gram matrices of every orientation (all rows for the NNLS stages, stage-2 rows for the LASSO):
    // they let the solver update the dual vector without sweeping the tile (amx_solver.hpp)
    lut->ldG = n_atoms <= 192 ? 192 : 256;            // (>= 64 atoms per lane-row of the solvers' column reads)
    const size_t gbytes = (size_t)ndirs * n_atoms * lut->ldG * sizeof(double);
    const size_t lds_tile = (size_t)nS * lut->ldA * sizeof(float);
    const int in_lds = lds_tile <= 160 * 1024 ? 1 : 0;
    const size_t lds = in_lds ? lds_tile : 0;
    HIPCHK(ctx, hipMalloc((void **)&lut->gram, gbytes));
    HIPCHK(ctx, hipMalloc((void **)&lut->gram_dwi, gbytes));
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_build_gram), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_build_gram, dim3(ndirs), dim3(512), lds, nullptr, (const float *)lut->tiles, lut->tile_stride, nS, lut->ldA, n_atoms, (const unsigned char *)nullptr, lut->ldG, lut->gram, in_lds);
    hipLaunchKernelGGL(k_build_gram, dim3(ndirs), dim3(512), lds, nullptr, (const float *)lut->tiles, lut->tile_stride, nS, lut->ldA, n_atoms, (const unsigned char *)lut->rowdwi, lut->ldG, lut->gram_dwi, in_lds);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipDeviceSynchronize());
    // compressed basis of every orientation: support seeds of the NNLS stages (amx_seed.hpp)
    // (ex-vivo dictionaries too: the dot atom -- a column of ones -- is one more atom; their stage-2 products always take the exact
    //  pass, s2_derive = 0: y2 = y - x_iso iso - x_dot is not a function of x_iso alone)
    if ((rc = amx_build_basis(ctx, lut))) { amx_lut_destroy(lut); return rc; }
    *out = lut;
    return AMX_OK;
}

int amx_lut_upload_freewater(amx_ctx *ctx, const float *D, const float *CSF, const int16_t *htable,
                             int n_perp, int n_iso, int ndirs, int nS, amx_lut **out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!D || !CSF || !htable || !out || n_perp <= 0 || n_iso <= 0 || ndirs <= 0 || nS <= 0)
        return amx_bad(ctx, "amx_lut_upload_freewater: bad argument");
    const int n_atoms = n_perp + n_iso;
    if (n_atoms > kBigMaxAtoms || nS > 512) return amx_bad(ctx, "amx_lut_upload_freewater: unsupported size (n_atoms <= 256, nS <= 512)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    amx_lut *lut = new_lut(ctx, 2, nS, n_atoms, ndirs);
    lut->n_perp = n_perp; lut->n_iso = n_iso;
    int rc;
    std::vector<int> ones(n_iso, 0);
    if ((rc = build_tiles(ctx, lut, D, (size_t)n_perp * ndirs * nS, CSF, (size_t)n_iso * nS, ones, n_perp))) { amx_lut_destroy(lut); return rc; }
    std::vector<short> ht(htable, htable + 181 * 181);
    if ((rc = amx_upload(ctx, &lut->htable, ht.data(), ht.size()))) { amx_lut_destroy(lut); return rc; }
    if (amx_big_dictionary(lut) && (rc = amx_build_big_gram(ctx, lut))) { amx_lut_destroy(lut); return rc; }      // (more than 64 atoms: k_enet_big works on A'A)
    *out = lut;
    return AMX_OK;
}

int amx_lut_upload_sandi(amx_ctx *ctx, const double *signal, const double *norms, const double *Rs,
                         const double *d_in, const double *d_isos, int nS, int n_rs, int n_in,
                         int n_iso, amx_lut **out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!signal || !norms || !Rs || !d_in || !d_isos || !out || nS <= 0 || n_rs < 0 || n_in < 0 || n_iso < 0)
        return amx_bad(ctx, "amx_lut_upload_sandi: bad argument");
    const int n_atoms = n_rs + n_in + n_iso;
    if (n_atoms <= 0 || n_atoms > kBigMaxAtoms || nS > 512) return amx_bad(ctx, "amx_lut_upload_sandi: unsupported size (n_atoms <= 256, nS <= 512)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    amx_lut *lut = new_lut(ctx, 3, nS, n_atoms, 1);
    lut->n_rs = n_rs; lut->n_in = n_in; lut->n_isos = n_iso;
    std::vector<double> tile((size_t)lut->tile_stride + 8, 0.0);
    for (int j = 0; j < n_atoms; j++)
        for (int i = 0; i < nS; i++) tile[(size_t)i * lut->ldA + j] = signal[(size_t)j * nS + i];   // col-major in
    int rc;
    double *dt = nullptr;
    if ((rc = amx_upload(ctx, &dt, tile.data(), tile.size())) || (rc = amx_upload(ctx, &lut->norms, norms, (size_t)n_atoms)) ||
        (rc = amx_upload(ctx, &lut->Rs, Rs, (size_t)(n_rs ? n_rs : 1))) || (rc = amx_upload(ctx, &lut->d_in, d_in, (size_t)(n_in ? n_in : 1))) ||
        (rc = amx_upload(ctx, &lut->d_isos, d_isos, (size_t)(n_iso ? n_iso : 1)))) { lut->tiles = dt; amx_lut_destroy(lut); return rc; }
    lut->tiles = dt;
    if (amx_big_dictionary(lut) && (rc = amx_build_big_gram(ctx, lut))) { amx_lut_destroy(lut); return rc; }
    *out = lut;
    return AMX_OK;
}

int amx_lut_upload_czb(amx_ctx *ctx, const float *wmr, const float *wmh, const float *iso, const double *Rs,
                       const int16_t *htable, int n_rs, int n_perp, int n_iso, int ndirs, int nS, amx_lut **out)
{
    if (!ctx) return AMX_E_BADARG;
    if (!wmr || !wmh || !iso || !Rs || !htable || !out || n_rs <= 0 || n_perp <= 0 || n_iso <= 0 || ndirs <= 0 || nS <= 0)
        return amx_bad(ctx, "amx_lut_upload_czb: bad argument");
    const int n_atoms = n_rs + n_perp + n_iso;
    if (n_atoms > kBigMaxAtoms || nS > 512) return amx_bad(ctx, "amx_lut_upload_czb: unsupported size (n_atoms <= 256, nS <= 512)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    amx_lut *lut = new_lut(ctx, 4, nS, n_atoms, ndirs);
    lut->n_rs = n_rs; lut->n_perp = n_perp; lut->n_iso = n_iso;
    int rc;
    // columns: cylinders, zeppelins (both per orientation), balls (models.pyx:608-610)
    std::vector<float> rot((size_t)(n_rs + n_perp) * ndirs * nS);
    memcpy(rot.data(), wmr, (size_t)n_rs * ndirs * nS * sizeof(float));
    memcpy(rot.data() + (size_t)n_rs * ndirs * nS, wmh, (size_t)n_perp * ndirs * nS * sizeof(float));
    std::vector<int> ones(n_iso, 0);
    if ((rc = build_tiles(ctx, lut, rot.data(), rot.size(), iso, (size_t)n_iso * nS, ones, n_rs + n_perp))) { amx_lut_destroy(lut); return rc; }
    std::vector<short> ht(htable, htable + 181 * 181);
    if ((rc = amx_upload(ctx, &lut->htable, ht.data(), ht.size())) || (rc = amx_upload(ctx, &lut->Rs, Rs, (size_t)n_rs))) { amx_lut_destroy(lut); return rc; }
    // Gram matrices of every orientation: the solver works on A'A + lambda2 I (amx_gram_solver.hpp; more than 64 atoms: amx_enet_big.hip)
    if (amx_big_dictionary(lut)) {
        if ((rc = amx_build_big_gram(ctx, lut))) { amx_lut_destroy(lut); return rc; }
        *out = lut;
        return AMX_OK;
    }
    lut->ldG = kCzbLdG;
    const size_t gbytes = (size_t)ndirs * n_atoms * lut->ldG * sizeof(double);
    const size_t lds = (size_t)nS * lut->ldA * sizeof(float);
    if (hipMalloc((void **)&lut->gram, gbytes) != hipSuccess) { amx_lut_destroy(lut); return amx_bad(ctx, "amx_lut_upload_czb: out of device memory"); }
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_build_gram), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_build_gram, dim3(ndirs), dim3(512), lds, nullptr, (const float *)lut->tiles, lut->tile_stride, nS, lut->ldA, n_atoms, (const unsigned char *)nullptr, lut->ldG, lut->gram);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipDeviceSynchronize());
    *out = lut;
    return AMX_OK;
}

}  // extern "C"
