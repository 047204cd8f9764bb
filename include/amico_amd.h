/*
 * amico_amd.h -- C ABI of the MI355X-native AMICO per-voxel fitter (libamico_amd.so).
 *
 * Drop-in boundary for the hot path `model.fit(evaluation)` of daducci/AMICO v2.1.0.
 * The reference has no C ABI for this path: its native boundary is Cython `cdef` calls
 * (amico/lut.pxd:4 `dir_to_lut_idx`; amico/models.pyx:18 `cyspams.interfaces.nnls/lasso`)
 * made from the `_fit` hot loops (models.pyx:816-991 NODDI, 1168-1286 FreeWater,
 * 1509-1627 SANDI).  Each entry point below cites the reference interface it replaces.
 *
 * Conventions: plain pointers + sizes, no C++/torch types; every call returns an int
 * status (0 = ok, negative = error, see AMX_E_*); the library never keeps host pointers
 * after a call returns; device memory is owned by amx_ctx / amx_lut handles.
 * Arrays use the reference's layouts and dtypes (C-order, float64 signals / maps).
 * Threading: the calls on one context, and on the dictionary handles made from it, are serialised by the caller, like the
 * reference's single `model.fit` call per Evaluation; the FreeWater / SANDI handles cache small per-dictionary tables for the
 * last (lambda1, lambda2) they were fitted with and rebuild them when the solver parameters change.
 */
#ifndef AMICO_AMD_H
#define AMICO_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define AMX_OK              0
#define AMX_E_BADARG       -1   /* NULL / negative size / unsupported protocol size          */
#define AMX_E_HIP          -2   /* HIP runtime error (message in amx_last_error)             */
#define AMX_E_DIR_OOB      -3   /* lut.pyx:352-354 "index out of bounds" (voxel in last_error) */
#define AMX_E_OVERFLOW     -4   /* a voxel needed more active atoms than the kernels support  */
#define AMX_E_NODEVICE     -5   /* no HIP device / wrong architecture                         */

/* flags of the *_fit calls (Evaluation.get_config(...) switches read by BaseModel.fit,
 * models.pyx:214-217, 797, 1149) */
#define AMX_F_RMSE          1u  /* doComputeRMSE        -> out_rmse   f64[n_vox]      */
#define AMX_F_NRMSE         2u  /* doComputeNRMSE       -> out_nrmse  f64[n_vox]      */
#define AMX_F_MODULATED     4u  /* doSaveModulatedMaps  -> out_mod    f64[n_vox][2]   */
#define AMX_F_CORRECTED     8u  /* doSaveCorrectedDWI   -> out_ycorr  f64[n_vox][nS]  */
#define AMX_F_DEBUG_X      16u  /* solver coefficients  -> the buffer registered with amx_set_debug_x */
#define AMX_F_FW_ISO       32u  /* FreeWater only: the isotropic coefficients -> the buffer registered with amx_set_fw_iso */

typedef struct amx_ctx amx_ctx;   /* one per process+GPU: stream-ordered workspace, error state */
typedef struct amx_lut amx_lut;   /* device-resident dictionary (KERNELS) of one model          */

int  amx_version(void);
/* "amico_amd <version> csrc <16 hex digits>": the digits are sha256 of the library's sources (the .hip and .hpp files of amico_amd/csrc and this
 * header, concatenated in name order) as they were when the library was BUILT -- amico_amd._capi.source_id() takes the same hash of
 * the sources in the tree, so a stale .so, or a profile summary taken from other kernels (profiles/pmc_traffic.json carries the id
 * of the build it measured), is detected instead of trusted.  Static storage. */
const char *amx_build_id(void);
/* HIP devices this process may create contexts on: the largest gfx950 device number + 1 (0: none).  The reference's caller is ONE process
 * (core.py:465-466: results = self.model.fit(self)) whose fit spreads its voxels over `nthreads` host threads in contiguous chunks
 * (models.pyx:204-211); the MI355X counterpart of that is one context per device of the node, driven by one host thread each, on contiguous
 * shards of the caller's arrays -- amico_amd.models does exactly that when AMX_DEVICES=all (or a list) is set: every call of this ABI sets its
 * context's device for the calling thread, contexts share nothing, and calls on DIFFERENT contexts may run concurrently from different threads. */
int  amx_device_count(void);
/* A context that fits ONE SHARD of a larger call (several contexts sharing a fit, see above): the host-buffer calls that follow choose their
 * paths -- seeded chain or not, kernel builds, rescue pass -- by `total`, the size of the whole call, not by the shard's, so that a voxel is
 * settled by the same arithmetic whichever device it lands on and however many there are (bit-identical maps).  0 = off (the default). */
int  amx_set_call_voxels(amx_ctx *ctx, int64_t total);
/* device < 0: current HIP device.  Fails with AMX_E_NODEVICE when no gfx950 GPU is visible. */
int  amx_ctx_create(int device, amx_ctx **out);
void amx_ctx_destroy(amx_ctx *ctx);
/* last error text of this ctx ("" if none); valid until the next call on ctx */
const char *amx_last_error(amx_ctx *ctx);

/* ---- dictionaries: replace the per-thread re-materialisation of KERNELS in _fit
 *      (models.pyx:840-847 NODDI, 1190-1191 FreeWater, 1527-1528 SANDI) by ONE upload.   */

/* NODDI.  KERNELS['wm'] f32[n_wm][ndirs][nS], ['iso'] f32[nS], ['norms'] f64[dwi][n_wm]
 * (rows identical, models.pyx:781-784), ['icvf'],['kappa'] f32[n_wm] (models.pyx:763-789);
 * htable int16[181*181] (lut.pyx:71-91); dwi_idx = scheme.dwi_idx int64[dwi_count].
 * Any shape the reference's loop takes (models.pyx:825-861) up to nS <= 512 volumes and n_wm + 1 (+ 1) <= 256 atoms.  The seeded
 * chain (seed solvers -> Gram-space certificates) covers every protocol of that range with <= 160 atoms; a dictionary tile that does
 * not fit a compute unit's LDS (288 volumes x 145 atoms float32 = 167 KB: an HCP-style acquisition) is read from HBM / L2 by the
 * wavefront-per-voxel kernels instead -- slower for the few per cent of voxels that reach them, same results.                      */
int amx_lut_upload_noddi(amx_ctx *ctx, const float *wm, const float *iso, const double *norms,
                         const float *icvf, const float *kappa, const int16_t *htable,
                         const int64_t *dwi_idx, int n_wm, int ndirs, int nS, int dwi_count,
                         int is_exvivo, amx_lut **out);
/* FreeWater.  KERNELS['D'] f32[n_perp][ndirs][nS], ['CSF'] f32[n_iso][nS] (models.pyx:1122-1123).
 * Any shape the reference's loop takes (models.pyx:1231-1276) up to n_perp + n_iso <= 256 atoms, nS <= 512 volumes.  Up to 64 atoms the
 * dictionary is its tiles; beyond that -- a finer grid of d_perps in model.set() -- the upload also builds the Gram matrices A_d'A_d of every
 * orientation in HBM (f64, ndirs * n_atoms^2 * 8 bytes: 262 MB at 500 x 256 atoms; "out of device memory" is AMX_E_BADARG) and the fits
 * take the dense route of csrc/amx_enet_big.hip (k_enet_big: a workgroup per voxel, every output and flag of the smaller dictionaries).
 * The same holds for SANDI and CylinderZeppelinBall below; the dictionary's shape alone selects the route. */
int amx_lut_upload_freewater(amx_ctx *ctx, const float *D, const float *CSF, const int16_t *htable,
                             int n_perp, int n_iso, int ndirs, int nS, amx_lut **out);
/* SANDI.  KERNELS['signal'] f64 column-major [nS][n_atoms], ['norms'] f64[n_atoms]
 * (models.pyx:1456-1482); Rs, d_in, d_isos = model parameters used by the maps (:1540-1542).
 * n_atoms <= 256, nS <= 512: the direction-averaged shells (6 values) as well as the acquisition itself (doDirectionalAverage off, the
 * reference's default: 306 volumes).  Protocols of more than 128 volumes are fitted in Gram space (A'y of every voxel on the fp64 matrix
 * cores, then H = A'A + lambda2 I per voxel: csrc/amx_sandi_long.hip) and need lambda2 >= 1e-9 -- an isotropic dictionary has rank
 * <= shells + 1 < n_atoms, so without the ridge the optimum is not unique; amx_sandi_fit* answer AMX_E_BADARG there (whatever the number of atoms).
 * amx_last_kernel_ms of such a fit: 1 = the solver kernel, 2 = the projection. */
int amx_lut_upload_sandi(amx_ctx *ctx, const double *signal, const double *norms, const double *Rs,
                         const double *d_in, const double *d_isos, int nS, int n_rs, int n_in,
                         int n_iso, amx_lut **out);
/* CylinderZeppelinBall.  KERNELS['wmr'] f32[n_rs][ndirs][nS] (cylinders), ['wmh'] f32[n_perp][ndirs][nS] (zeppelins),
 * ['iso'] f32[n_iso][nS] (balls) (models.pyx:488-520); Rs = model.Rs f64[n_rs] in metres, used by the maps (:627).
 * n_rs + n_perp + n_iso <= 256 atoms, nS <= 512 volumes (more than 64 atoms: see FreeWater above). */
int amx_lut_upload_czb(amx_ctx *ctx, const float *wmr, const float *wmh, const float *iso, const double *Rs,
                       const int16_t *htable, int n_rs, int n_perp, int n_iso, int ndirs, int nS, amx_lut **out);
void amx_lut_destroy(amx_lut *lut);

/* ---- lut.pxd:4  cdef int dir_to_lut_idx(double[::1] direction, short[::1] hash_table)
 * batched; dirs f64[n][3] (host, NOT modified -- the reference flips it in place,
 * lut.pyx:335-338); out_idx int32[n].  AMX_E_DIR_OOB mirrors the RuntimeError.             */
int amx_dir_to_lut_idx(amx_ctx *ctx, const amx_lut *lut, const double *dirs, int64_t n,
                       int32_t *out_idx);

/* ---- model.fit hot loops, HOST buffers in / out (H2D + kernels + D2H, blocking; the copies of large
 * inputs overlap with the solver, in batches -- and the maps of finished batches go home while later batches are still being solved: when a
 * call returns an error (AMX_E_DIR_OOB from a later batch, a HIP error) the output arrays may already hold the results of the batches before it.
 * The reference raises before it returns anything (models.pyx:904 inside the loop that fills `estimates`, which is then lost with the
 * exception); the Python mirror does the same: its wrappers raise and the arrays are unreachable.
 * y f64[n_vox][nS] (evaluation.y, core.py:451-452), dirs f64[n_vox][3] (evaluation.DIRs).
 * lambda1 >= 0, lambda2 >= 0 like cyspams' lasso (lambda2 = 0 runs the QR solver in A-space).  */

/* NODDI._fit models.pyx:816-991: estimates f64[n_vox][3 (+1 ex-vivo)] = NDI, ODI, FWF(, dot) */
int amx_noddi_fit(amx_ctx *ctx, const amx_lut *lut, const double *y, const double *dirs,
                  int64_t n_vox, double lambda1, double lambda2, unsigned flags,
                  double *out_estimates, double *out_rmse, double *out_nrmse, double *out_mod);
/* FreeWater._fit models.pyx:1168-1286: estimates f64[n_vox][2 (Human) | 4 (Mouse)] */
int amx_freewater_fit(amx_ctx *ctx, const amx_lut *lut, const double *y, const double *dirs,
                      int64_t n_vox, double lambda1, double lambda2, int is_mouse, unsigned flags,
                      double *out_estimates, double *out_rmse, double *out_nrmse, double *out_ycorr);
/* SANDI._fit models.pyx:1509-1627: estimates f64[n_vox][6] */
int amx_sandi_fit(amx_ctx *ctx, const amx_lut *lut, const double *y, int64_t n_vox,
                  double lambda1, double lambda2, unsigned flags,
                  double *out_estimates, double *out_rmse, double *out_nrmse);

/* CylinderZeppelinBall._fit models.pyx:526-652: estimates f64[n_vox][3] = v, a, d.  Any lambda2 >= 0 like the reference's
 * lasso (models.pyx:439, 615): the default 4.0 makes the Gram-space solver the right tool, lambda2 < 1e-6 runs the thin-QR
 * solver in A-space.  (The model's `isExvivo`, which the reference never defines, is not a parameter here.) */
int amx_czb_fit(amx_ctx *ctx, const amx_lut *lut, const double *y, const double *dirs, int64_t n_vox,
                double lambda1, double lambda2, unsigned flags,
                double *out_estimates, double *out_rmse, double *out_nrmse);
int amx_czb_fit_f32(amx_ctx *ctx, const amx_lut *lut, const float *y, const double *dirs, int64_t n_vox,
                    double lambda1, double lambda2, unsigned flags,
                    double *out_estimates, double *out_rmse, double *out_nrmse);
int amx_czb_fit_device(amx_ctx *ctx, const amx_lut *lut, const double *d_y, const double *d_dirs,
                       int64_t n_vox, double lambda1, double lambda2, unsigned flags,
                       double *d_estimates, double *d_rmse, double *d_nrmse, void *hip_stream);

/* The same three calls with FLOAT32 signals: the image is float32 in the reference (core.py:136) and only cast to
 * float64 when the masked voxels are gathered (core.py:451), so a float32 `y` carries the same values in half the PCIe
 * bytes; it is widened on the GPU and every result is identical to the float64 call.                           */
int amx_noddi_fit_f32(amx_ctx *ctx, const amx_lut *lut, const float *y, const double *dirs,
                      int64_t n_vox, double lambda1, double lambda2, unsigned flags,
                      double *out_estimates, double *out_rmse, double *out_nrmse, double *out_mod);
int amx_freewater_fit_f32(amx_ctx *ctx, const amx_lut *lut, const float *y, const double *dirs,
                          int64_t n_vox, double lambda1, double lambda2, int is_mouse, unsigned flags,
                          double *out_estimates, double *out_rmse, double *out_nrmse, double *out_ycorr);
int amx_sandi_fit_f32(amx_ctx *ctx, const amx_lut *lut, const float *y, int64_t n_vox,
                      double lambda1, double lambda2, unsigned flags,
                      double *out_estimates, double *out_rmse, double *out_nrmse);

/* Progress of the host-buffer calls: models.pyx:28-43, 981 keep a per-thread voxel counter that ProgressBar polls
 * (util.py); here `callback(done, total, user)` is called from the calling thread as batches of voxels complete (large
 * inputs are fitted in batches: a first one of 131 072 voxels, then equal parts of at most 393 216 voxels) and once with done == total at the end.  NULL unregisters.
 * The device-pointer calls below only ENQUEUE the fit: there the callback is a host function on the stream (hipLaunchHostFunc),
 * i.e. it is called from a HIP runtime thread when the work before it has finished -- after each of NODDI's three stages
 * (done = n/3, 2n/3, n) and at the end of a FreeWater / SANDI / CylinderZeppelinBall fit (done = n).  It must not call back
 * into this library.                                                                                                        */
int amx_set_progress(amx_ctx *ctx, void (*callback)(int64_t done, int64_t total, void *user), void *user);

/* ---- the same with DEVICE buffers (inputs already resident in HBM, e.g. torch tensors'
 * data_ptr()); work is enqueued on `hip_stream` (a hipStream_t, NULL = default stream) and
 * the call returns without synchronising.  amx_sync_status() waits for the stream and
 * returns the status of everything enqueued since the previous amx_sync_status().          */
int amx_noddi_fit_device(amx_ctx *ctx, const amx_lut *lut, const double *d_y, const double *d_dirs,
                         int64_t n_vox, double lambda1, double lambda2, unsigned flags,
                         double *d_estimates, double *d_rmse, double *d_nrmse, double *d_mod,
                         void *hip_stream);
int amx_freewater_fit_device(amx_ctx *ctx, const amx_lut *lut, const double *d_y,
                             const double *d_dirs, int64_t n_vox, double lambda1, double lambda2,
                             int is_mouse, unsigned flags, double *d_estimates, double *d_rmse,
                             double *d_nrmse, double *d_ycorr, void *hip_stream);
int amx_sandi_fit_device(amx_ctx *ctx, const amx_lut *lut, const double *d_y, int64_t n_vox,
                         double lambda1, double lambda2, unsigned flags, double *d_estimates,
                         double *d_rmse, double *d_nrmse, void *hip_stream);
/* The same with float32 signals in HBM -- the dtype the image has before core.py:451-452 widen it (core.py:136: float32), so
 * the maps are bit-identical to the float64 calls on the widened values.  NODDI (A'y GEMM, left-over kernels), every
 * wavefront-per-voxel kernel, CylinderZeppelinBall and FreeWater's matrix-core projection read the float32 rows in place (FreeWater:
 * 260 instead of 520 bytes per voxel); for the remaining lane kernels (FreeWater with error maps / AMX_F_CORRECTED, SANDI) a float64
 * copy is made on the device first.                                                                                            */
int amx_noddi_fit_device_f32(amx_ctx *ctx, const amx_lut *lut, const float *d_y, const double *d_dirs,
                             int64_t n_vox, double lambda1, double lambda2, unsigned flags,
                             double *d_estimates, double *d_rmse, double *d_nrmse, double *d_mod, void *hip_stream);
int amx_freewater_fit_device_f32(amx_ctx *ctx, const amx_lut *lut, const float *d_y, const double *d_dirs, int64_t n_vox,
                                 double lambda1, double lambda2, int is_mouse, unsigned flags, double *d_estimates,
                                 double *d_rmse, double *d_nrmse, double *d_ycorr, void *hip_stream);
int amx_sandi_fit_device_f32(amx_ctx *ctx, const amx_lut *lut, const float *d_y, int64_t n_vox, double lambda1, double lambda2,
                             unsigned flags, double *d_estimates, double *d_rmse, double *d_nrmse, void *hip_stream);
int amx_czb_fit_device_f32(amx_ctx *ctx, const amx_lut *lut, const float *d_y, const double *d_dirs, int64_t n_vox,
                           double lambda1, double lambda2, unsigned flags, double *d_estimates, double *d_rmse,
                           double *d_nrmse, void *hip_stream);
int amx_sync_status(amx_ctx *ctx, void *hip_stream);

/* ---- the solvers' own output: the coefficient vectors `x` that cyspams.interfaces.nnls / lasso hand back to
 * _fit (models.pyx:911, 926, 940, 1238, 1569: `x` fully written, exact zeros off the support).  The reference keeps
 * them internal; here they are observable so that tests can certify the DEVICE solution itself (KKT conditions,
 * supports), not only the maps derived from it.  d_x is a DEVICE buffer the caller owns (zero it first; NULL
 * unregisters).  Every later *_fit / *_fit_device call on this ctx whose flags carry AMX_F_DEBUG_X fills it:
 *   NODDI      f64[n_vox][3][n_atoms]: row 0 = stage-1 NNLS over all atoms (wm..., [dot,] iso); row 1 = LASSO
 *              coefficients of the wm atoms (column-normalised dictionary, models.pyx:917-921) followed by the
 *              stage-1 iso (dot) coefficients (the reference reuses one array); row 2 = the debiased x (:940-942)
 *   FreeWater  f64[n_vox][n_atoms]    the lasso solution (models.pyx:1238)
 *   SANDI      f64[n_vox][n_atoms]    the lasso solution rescaled by KERNELS['norms'] (models.pyx:1570-1571)   */
int amx_set_debug_x(amx_ctx *ctx, double *d_x);

/* ---- FreeWater's corrected DWI (models.pyx:1264-1274, core.py:488-498) without the fit leaving its fast kernels:
 *     y_corrected[i, j] = max(0, y[i, j] - sum_k CSF[k, j] x[i, n_perp + k])
 * needs only the one (Human) or two (Mouse) isotropic coefficients of each voxel.  A FreeWater fit whose flags carry AMX_F_FW_ISO
 * writes them -- entries n_perp .. n_atoms - 1 of the lasso solution, as the solver leaves them, before the maps normalise anything --
 * into d_xiso f64[n_vox][n_iso] at the voxel's own index (a DEVICE buffer the caller owns; NULL unregisters; a host-buffer call offsets
 * it per batch like the AMX_F_DEBUG_X buffer).  A voxel with a non-finite signal gets NaN, one skipped for an out-of-bounds direction 0,
 * as their maps do.  The flag selects no path: every kernel that writes FreeWater maps writes the coefficients, so a float32 fit
 * with it still runs k_freewater_fused in place on the float32 signals (AMX_F_CORRECTED keeps its own, slower route).  The flag without
 * a registered buffer, or on a fit of another model, is AMX_E_BADARG. */
int amx_set_fw_iso(amx_ctx *ctx, double *d_xiso);
/* The corrected signal from y and x_iso: one streaming kernel, lanes along the flattened (voxel, volume) index so that reads of y and
 * writes of the result are whole lines and voxels of few volumes share a wavefront.  Per sample, fp64 in the reference's order with
 * separately rounded products and sums (no fused multiply-add: the result equals the elementwise numpy expression bit for bit):
 *     fw = 0; for k: fw += (double)CSF[k][j] * x_iso[r][k];   yc = (double)y[r][j] - fw;   yc = yc < 0 ? 0 : yc   (NaN stays NaN)
 * CSF = the isotropic columns of the dictionary `lut` holds (at most 8).  Device pointers, enqueued on hip_stream, no synchronisation.
 * rows form:   d_y32 f32[n_vox][nS] or d_y64 f64[n_vox][nS] (exactly one is not NULL) -> d_ycorr f64[n_vox][nS]: what AMX_F_CORRECTED
 *              writes, one coalesced row per voxel. */
int amx_freewater_corrected_device(amx_ctx *ctx, const amx_lut *lut, const float *d_y32, const double *d_y64, const double *d_xiso,
                                   int64_t n_vox, double *d_ycorr, void *hip_stream);
/* (volume form: amx_prep_corrected_device, beside amx_prep_scatter_device below) */

/* ---- the signal the fitted model predicts, y_est = A x: what _compute_rmse / _compute_nrmse take the residual of and then drop
 * (models.pyx:47-71, called at :640, :971, :1259, :1615).  No counterpart in the reference's results; here it is made from what a fit
 * leaves in HBM -- the dictionary `lut` and the coefficient vectors AMX_F_DEBUG_X wrote (amx_set_debug_x) -- by one streaming kernel:
 *     y_est[i][s] = sum_j A_i[s][j] * x_i[j]
 *   NODDI      A_i = un-normalised [wm(lut_idx) | (dot) | iso], x_i = the debiased coefficients (row 2 of the AMX_F_DEBUG_X layout)
 *   FreeWater  A_i = [D(lut_idx) | CSF],                         x_i = the lasso solution
 *   SANDI      A_i = KERNELS['signal'],                          x_i = the coefficients rescaled by `norms` (the quirk of
 *              models.pyx:1570-1571 that the error maps reproduce: the prediction is the thing RMSE is the residual of)
 *   CZB        A_i = [wmr | wmh | iso] of the orientation,       x_i = the lasso solution
 * Row i's coefficients are d_x[i * x_stride + x_offset + j], j < n_atoms, counted in doubles: 3 * n_atoms and 2 * n_atoms for NODDI on
 * the debug buffer, n_atoms and 0 for the other models (and for a plain [n][n_atoms] buffer).  d_dirs f64[n_vox][3]: the directions
 * the fit was given (lut.pyx:316-356 picks the orientation); NULL for SANDI, which has one dictionary.
 * Arithmetic, per sample: fp64, atoms in ascending order, every product and every sum rounded on its own (no fused multiply-add):
 *     acc = 0; for j: acc = acc + (double)A[s][j] * x[j]
 * bit for bit; atoms whose coefficient is exactly 0 are skipped (adding +-0 changes nothing), a NaN coefficient is not zero: it makes the
 * whole row NaN, as that voxel's maps are.  A voxel whose direction is out of bounds gets a row of zeros, as its maps do (and the next
 * amx_sync_status reports it, as after the fit).  Coefficient vectors of any density are computed in full: the kernel keeps up to 16
 * non-zeros per voxel on chip and walks the dense vector for a voxel that has more.
 * Device pointers, enqueued on hip_stream, no synchronisation; calls on one ctx are to be enqueued on one stream at a time (they
 * share the ctx's LUT-index buffer, like the fits share its workspace).  AMX_E_BADARG with a message: a NULL pointer, d_dirs with a
 * dictionary of a model without directions or no d_dirs with any other, x_stride < x_offset + n_atoms.
 * rows form:   -> d_yest f64[n_vox][nS], one coalesced row per voxel. */
int amx_predict_device(amx_ctx *ctx, const amx_lut *lut, const double *d_x, int64_t x_stride, int64_t x_offset, const double *d_dirs,
                       int64_t n_vox, double *d_yest, void *hip_stream);
/* (volume form: amx_prep_predicted_device, beside amx_prep_corrected_device below) */

/* ---- wild (residual) bootstrap of the maps: a per-voxel standard error from B refits (no counterpart in the reference, whose
 * Evaluation.fit() gives one fit per subject).  Everything a replicate needs lies in HBM after a fit: the signals y, the directions,
 * the coefficients (AMX_F_DEBUG_X) and from them the prediction y_est = A x (amx_predict_device).  These three calls add the replicate
 * signal and the running moments; the refit itself is the ordinary amx_<model>_fit_device[_f32] on d_yb with the ORIGINAL fit's
 * directions (the tensor fit is not repeated: the uncertainty is conditional on the direction).  amico_amd/bootstrap.py drives them.
 * For replicate b = 0 .. B-1, voxel i of the call (+ the caller's first_voxel), volume j of nS:
 *     ctr = (first_voxel + i) * nS + j                                   (uint64, wraps)
 *     z   = seed + (b + 1) * 0x9E3779B97F4A7C15 + ctr * 0xD1B54A32D192ED03
 *     z   = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z   = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z   =  z ^ (z >> 31)
 *     s   = (z >> 63) ? -1 : +1                                          (Rademacher weight)
 *     v   = y_est[i][j] + s * ((double)y[i][j] - y_est[i][j])            (fp64; s * r is exact, so contraction cannot change v)
 *     y_b[i][j] = (v < 0) ? 0 : v                                        (the gather's clip, core.py:452; a NaN stays a NaN)
 * The sign depends on (seed, b, first_voxel + i, j, nS) only -- not on n_vox, the launch shape or how a call is split: first_voxel is
 * there so that a shard of a larger call reproduces that call's signs.  Every row is resampled, the b0 rows included.  y_b has the dtype
 * of y (float32: (float)v), so a replicate takes the same fit entry, and therefore the same kernels, as the original fit.
 * SANDI has no prediction of y (amx_predict_device gives the reference's quirk: rescaled coefficients on the normalised dictionary), so
 * its residuals mean nothing; the Python driver refuses it.
 * Device pointers, enqueued on hip_stream, no synchronisation; n_vox == 0 is a no-op.  AMX_E_BADARG with a message: a NULL buffer,
 * nS < 1, a negative n_vox / first_voxel / replicate, d_yb overlapping d_y or d_yest. */
int amx_bootstrap_resample_device(amx_ctx *ctx, const double *d_y, const double *d_yest, int64_t n_vox, int nS, int64_t first_voxel,
                                  uint64_t seed, int64_t replicate, double *d_yb, void *hip_stream);
int amx_bootstrap_resample_device_f32(amx_ctx *ctx, const float *d_y, const double *d_yest, int64_t n_vox, int nS, int64_t first_voxel,
                                      uint64_t seed, int64_t replicate, float *d_yb, void *hip_stream);
/* Welford's moments of the maps over the replicates, fp64, every operation rounded on its own (no fused multiply-add).  The t-th
 * replicate's maps (t = 1 .. B), for each of the n_elems = n_vox * n_maps elements m:
 *     d = m - mean;   mean += d / t;   M2 += d * (m - mean)
 * t = 1 takes mean = M2 = 0 without reading them, so neither buffer needs a memset.  A NaN map makes that element NaN from there on.
 * The three buffers must not overlap.  AMX_E_BADARG: t < 1, a NULL buffer, overlap. */
int amx_bootstrap_accumulate_device(amx_ctx *ctx, const double *d_maps, int64_t n_elems, int64_t t, double *d_mean, double *d_m2,
                                    void *hip_stream);
/* std = sqrt(M2 / (B - 1)) (division and root correctly rounded; d_std may be d_m2 itself).  AMX_E_BADARG for B < 2. */
int amx_bootstrap_std_device(amx_ctx *ctx, const double *d_m2, int64_t n_elems, int64_t B, double *d_std, void *hip_stream);

/* ---- diagnosis / tests of the support seeds (csrc/amx_seed.hpp; no counterpart in the reference): copies a workspace
 * buffer of the LAST NODDI fit of this ctx -- which = 0: voxel permutation int32[n] (bucket order), 1: projected signals
 * f64[n][12] (bucket order), 2: support seeds uint64[n] (bucket order; up to 8 atom ids, one per byte, >= 0xf0 = empty;
 * all ones = no seed), 3: projected clipped signals of the LASSO stage f64[n][12], 4: LASSO passive-set seeds uint64[n][4]
 * (bit j = atom j; word 3 all ones = no seed) -- or a table of the dictionary `lut` -- 10: orientation bases U
 * f64[ndirs][nS][12], 11: compressed dictionaries S = U'A f64[ndirs][n_atoms][12], 12 / 13: the same for the LASSO stage's
 * dictionary, f64[ndirs][nS][12] / f64[ndirs][n_wm][12] (the seed solver reads the first 8 components) -- into the HOST buffer dst (synchronises the device).
 * Further tables of `lut` (ldA = n_atoms rounded up to odd, tile_stride = nS * ldA rounded up to a multiple of 4):
 *   made at the upload
 *   14  tiles           f32 [ndirs][tile_stride] (SANDI: f64 [tile_stride]): tile[i * ldA + j] = atom j at volume i, padding 0.  Atoms of
 *                       NODDI: wm, (the dot, ex vivo), iso; FreeWater: D, CSF; CylinderZeppelinBall: wmr, wmh, iso
 *   15  gram            f64 [ndirs][n_atoms][ldG] = A'A, padding 0.  ldG: NODDI 192 (256 above 192 atoms), CylinderZeppelinBall 64,
 *                       any model of more than 64 atoms (n_atoms + 3) & ~3; the other dictionaries have none
 *   16  gram_dwi        the same over the stage-2 rows only (NODDI)
 *   17 / 18  screen_S / screen2_S    f32 [ndirs][12][192]: [d][j] = (float)S[j][d] of table 11 / 13, padding 0 (NODDI)
 *   19 / 20  screen_kappa / screen_kappa0,  21 / 22  screen2_kappa / screen2_kappa0    f64 [ndirs]: kappa0 = max_j ||a_j - U U'a_j||,
 *                       kappa = kappa0 + 2e-6 max_j ||a_j|| (stage 2: DWI rows, atoms times colscale)
 *   23  u2iso           f64 [ndirs][12] = U2'iso
 *   24  rowdwi          u8 [nS]: 1 = a row of stage 2;  25  colscale  f64 [n_atoms];  26  s2_derive  int32 [1]
 *   made by the first fit that reads them, for one lambda2 (refused until then)
 *   30  FreeWater       f64 [ndirs][W], N = 11 (n_atoms <= 11) or 12, NP = 12: A [nS][NP] | H^-1 [N][NP] | H [N][N], W = the sum rounded up to
 *                       even (that word is not written); padding atoms: 0 in A, identity in H
 *   31  CylinderZeppelinBall   f64 [ndirs][2 * 32 * 33 + 32 + 2 * 32 * nSp], nSp = 100 (nS <= 100) or 160: M [32][33] | H [32][33] | M 1 [32] |
 *                       B = M A' [32][nSp] | A' [32][nSp], all 0 outside the dictionary
 *   32  SANDI 6 x 15    f64 [15 * 22 + 15 * 6 + 16 + 8 * 16]: T [15][22] | G [15][6] | g0 [16] | A [6][16] | 32 unused words
 *   33  SANDI, more than 128 volumes   f64 [2 NP^2 + (NP / 16) KS 64], NP = n_atoms rounded up to 16, KS = 4 ceil(nS / 16): G [NP][NP] |
 *                       H [NP][NP] (identity on the padding) | A' in MFMA operand order: [(mt KS + s) 64 + l] = A[16 (s / 4) + 4 (l / 16) + s % 4][16 mt + l % 16]
 *   40  the Gram tables of a dense amx_dict, whose handle is passed in lut's place: f64 [n_dicts][n][ldG], ldG = n rounded up to odd, padding 0
 * AMX_E_BADARG with a message, and nothing copied: bytes larger than the table, a table that was never built, a handle of another model
 * or of another context.                                                                                                              */
int amx_debug_fetch(amx_ctx *ctx, const amx_lut *lut, int which, void *dst, size_t bytes);

/* ---- the solvers themselves, batched.  What the reference's FFI binds for this path is (models.pyx:18)
 *     from cyspams.interfaces cimport nnls, lasso
 *     nnls (&A[0,0], &y[i,0], m, n, &x[0], rnorm)                        models.pyx:911, 940
 *     lasso(&A[0,0], &y[i,0], m, n, 1, &x[0], lambda1, lambda2)          models.pyx:615, 926, 1238, 1569
 * one call per voxel, A column-major m x n with leading dimension m (a slice of the LUT), y one signal, x fully written.
 * A model injected through AMICO_WIP_MODELS (models.pyx:20-26) that writes its own _fit around these two calls reaches the GPU
 * solvers through the batched forms below: the dictionaries are uploaded once (one per LUT orientation, or a single one), every
 * voxel names its dictionary by index -- the `lut_idx` the reference computes per voxel (models.pyx:904) -- and all voxels are
 * solved by one call.
 *   amx_dict_upload    A f64[n_dicts][n][m]: n_dicts dictionaries, each column-major m x n with leading dimension m
 *                      (n <= 256 atoms, m <= 512 samples; a dictionary that does not fit a compute unit's LDS as fp64 is read from HBM / L2 instead: slower, same results; supports of up to 48 atoms)
 *   amx_nnls_batched   x_v = argmin_{x >= 0} ||A_d x - y_v||_2,  d = dict_idx[v] (NULL: the single dictionary),
 *                      Y f64[n_vox][m] -> X f64[n_vox][n] (exact zeros off the support), rnorm f64[n_vox] = ||A x - y||_2 or NULL
 *   amx_lasso_batched  x_v = argmin_{x >= 0} 1/2 ||y_v - A_d x||^2 + lambda1 sum(x) + lambda2/2 ||x||^2   (SPAMS lasso, mode
 *                      PENALTY, pos = true: what cyspams.lasso computes for p = 1; any lambda1, lambda2 >= 0)
 * Lawson-Hanson / its elastic-net form with a thin QR of the passive columns, one wavefront per voxel, strict Kuhn-Tucker stop
 * (csrc/amx_solver.hpp); a support of more than 48 atoms is beyond it (AMX_E_OVERFLOW -- AMICO's problems end at ~25).  A voxel with a non-finite signal gets NaN; an index outside [0, n_dicts) is reported like a bad
 * direction (AMX_E_DIR_OOB, the first offending voxel in the message) and its x stays zero.  The *_device forms take device
 * pointers and a hipStream_t and are asynchronous (amx_sync_status returns the status).
 * Supports of ANY size, opt-in per dictionary -- the reference's nnls / lasso have no cap below min(m, n):
 *   amx_dict_set_dense       on != 0: build the Gram matrices G_d = A_d'A_d on the GPU from the uploaded tiles (f64[n_dicts][n][ldG]: n^2
 *                            doubles per dictionary, and a build pass -- only the caller who needs dense supports pays for them) and mark the
 *                            dictionary.  On a marked dictionary the four batched calls never answer AMX_E_OVERFLOW for the size of a support:
 *                            the voxels the 48-atom pass cannot hold are solved by k_batched_big (csrc/amx_batched_big.hip: block principal
 *                            pivoting in Gram space, a workgroup per voxel, the result checked against the true residual), every other voxel
 *                            exactly as on an unmarked dictionary.  Idempotent; on == 0 frees the tables and clears the mark; a dictionary of
 *                            another ctx is AMX_E_BADARG; a failed allocation is AMX_E_HIP and leaves the dictionary unmarked.
 *                            amx_dict_destroy frees the tables.  An unmarked dictionary enqueues exactly what it did before.
 *   amx_batched_last_dense   of the last synchronised batched call: out[0] = voxels k_batched_big solved, out[1] = its pivoting steps
 *                            (factorisations) over all of them.                                                                          */
typedef struct amx_dict amx_dict;
int  amx_dict_upload(amx_ctx *ctx, const double *A, int m, int n, int n_dicts, amx_dict **out);
void amx_dict_destroy(amx_dict *dict);
int  amx_dict_set_dense(amx_ctx *ctx, amx_dict *dict, int on);
int  amx_batched_last_dense(amx_ctx *ctx, int64_t out[2]);
int amx_nnls_batched(amx_ctx *ctx, const amx_dict *dict, const int32_t *dict_idx, const double *y, int64_t n_vox,
                     double *x, double *rnorm);
int amx_lasso_batched(amx_ctx *ctx, const amx_dict *dict, const int32_t *dict_idx, const double *y, int64_t n_vox,
                      double lambda1, double lambda2, double *x);
int amx_nnls_batched_device(amx_ctx *ctx, const amx_dict *dict, const int32_t *d_dict_idx, const double *d_y, int64_t n_vox,
                            double *d_x, double *d_rnorm, void *hip_stream);
int amx_lasso_batched_device(amx_ctx *ctx, const amx_dict *dict, const int32_t *d_dict_idx, const double *d_y, int64_t n_vox,
                             double lambda1, double lambda2, double *d_x, void *hip_stream);

/* ---- next rows of the hot-path table (SURVEY.md section 8 f): the steps either side of model.fit ---- */

/* (f1) principal directions, core.py:431-436 + 456-458:
 *     DTI = dipy.reconst.dti.TensorModel(gtab, fit_method='OLS');  DIRs = np.squeeze(DTI.fit(y).directions)
 * i.e. per voxel  p = pinv(design_matrix(gtab)) @ log(max(y, min_signal)),  D = lower-triangular p[0:6]
 * (Dxx Dxy Dyy Dxz Dyz Dzz), direction = eigenvector of the largest eigenvalue of D (dipy/reconst/dti.py:
 * TensorModel.fit, ols_fit_tensor, decompose_tensor; dipy>=1.4.1, requirements.txt:3).  The sign of an
 * eigenvector is not defined (LAPACK's choice in the reference); dir_to_lut_idx folds it away (lut.pyx:335-338).
 * inv_design f64[7][nS] (host, C-order) = numpy.linalg.pinv(design matrix) -- one-off per scheme, host side;
 * min_signal = dipy's MIN_POSITIVE_SIGNAL (1e-4) unless the caller configured another.                        */
typedef struct amx_dti amx_dti;
int  amx_dti_create(amx_ctx *ctx, const double *inv_design, int nS, double min_signal, amx_dti **out);
/* The reference hands the configuration's DTI_fit_method to TensorModel (core.py:419-420, 436).  Besides 'OLS' | 'LS' above:
 *   WLS  (dipy/reconst/dti.py: wls_fit_tensor)  X = design matrix, s = max(y, min_signal):  p_ols = pinv(X) log s;
 *        w = exp(X p_ols), the signal the OLS fit predicts;  p = argmin sum_i w_i^2 (log s_i - X_i p)^2
 *        (dipy: pinv(X * w[:, None]) @ (w * log s)); direction from p[0:6] as above.
 *   NLLS (dipy/reconst/dti.py: nlls_fit_tensor, weighting=None)  p = argmin sum_i (s_i - exp(X_i p))^2, the local minimum
 *        next to the linear fit.  dipy runs MINPACK's Levenberg-Marquardt from a linear fit with an analytic Jacobian (which
 *        linear fit has changed between dipy releases; the minimum does not depend on it except in pathological voxels) and
 *        keeps the starting parameters when the solve fails.  Here: Levenberg-Marquardt from the WLS solution, run until the
 *        cost stops moving in fp64 -- MINPACK at dipy's default tolerances stops earlier, so the two agree to MINPACK's
 *        stopping rule, not to rounding.  A voxel that reaches the trip cap or a non-finite value keeps the WLS parameters
 *        and is counted (amx_dti_last_unconverged); no error is raised, as in the reference.
 *   RESTORE ('RT' | 'RESTORE' | 'restore'; dipy/reconst/dti.py: restore_fit_tensor; Chang, Jones & Pierpaoli 2005)  needs the
 *        noise level sigma > 0 in the units of y, one scalar per estimator (amx_dti_create_robust): the reference's own call passes
 *        none and raises inside dipy.  Per voxel:
 *          1. p1 = the NLLS fit above, by the arithmetic above (dipy's 1 / sigma^2 weights do not move the minimum)
 *          2. r = s - exp(X p1);  no |r_i| > 3 sigma: done, p = p1, 0 outliers
 *          3. the Geman-McClure fit as a fixed point, from p1.  One trip: r at p;  C = max(1.4826 median|r - median(r)|,
 *             1e-6 sigma) (numpy's median);  w_i = 1 / (r_i^2 + C^2) / mean(w);  ONE Levenberg-Marquardt trial on
 *             sum w_i (s_i - exp(X_i p))^2 with w frozen (J = exp(X p) (.) X, (J'WJ + lam diag) d = J'Wr, accepted when the
 *             frozen-weight cost does not rise; lam as in NLLS: 1e-3 at the start, x 0.1 on accept with floor 1e-12, x 10 on reject, give
 *             up above 1e12).  Converged when an accepted step has max_i |X_i d| <= 1e-10.  At most 1024 trips; a voxel at the cap
 *             or giving up keeps its last accepted iterate and is counted (amx_dti_last_robust).
 *          4. r = s - exp(X p2), O = {i : |r_i| > 3 sigma}.  O empty: p = p2.  Fewer than 7 samples outside O: p = p2, counted.
 *             Otherwise the samples outside O are fitted anew: OLS, WLS and NLLS as above over those samples.  A failed NLLS keeps
 *             the WLS parameters of those samples, a failed OLS (a singular system) keeps p2; both are counted in
 *             amx_dti_last_unconverged.
 *          5. tensor -> direction (evals, scalars) as above;  outliers = |O|, 0 for a voxel that ended at step 2.
 *        This is restore_fit_tensor in structure.  Two differences are deliberate.  Step 3 is a defined fixed point, the
 *        iteratively reweighted fit of Chang et al.: dipy hands MINPACK a cost whose weights move under it, with a Jacobian that
 *        ignores them.  And every fit runs to its minimum, not to MINPACK's default tolerances.  With a sigma so large that no
 *        sample is ever an outlier the outputs are NLLS's, bit for bit.  Schemes of up to 512 volumes.
 * design f64[nS][7] (host, C-order) = dipy.reconst.dti.design_matrix(gtab), needed for WLS / NLLS (may be NULL for OLS);
 * both fits run in fp64 on the design matrix with its columns scaled to unit max-abs.  Schemes whose two [nS][7] tables and
 * signal tile exceed the 160 KB of LDS are refused by amx_dti_directions* ("scheme too long").                              */
enum { AMX_DTI_OLS = 0, AMX_DTI_WLS = 1, AMX_DTI_NLLS = 2, AMX_DTI_RESTORE = 3 };
int  amx_dti_create_method(amx_ctx *ctx, const double *design, const double *inv_design, int nS, double min_signal, int method,
                           amx_dti **out);
/* the RESTORE estimator (amx_dti_create_method refuses AMX_DTI_RESTORE: it has no sigma); AMX_E_BADARG unless sigma is finite and > 0 */
int  amx_dti_create_robust(amx_ctx *ctx, const double *design, const double *inv_design, int nS, double min_signal, double sigma,
                           amx_dti **out);
void amx_dti_destroy(amx_dti *h);
/* voxels of the last NLLS / RESTORE call on this handle that kept their starting parameters (0 for the other methods; RESTORE: of
 * step 1 or of step 4); waits for that call */
int amx_dti_last_unconverged(amx_ctx *ctx, const amx_dti *h, int64_t *out);
/* Levenberg-Marquardt trips of the last NLLS / RESTORE call: summed over its voxels, and summed over the trips their wavefronts ran
 * for them (a voxel that has converged idles until the last of the 8 voxels of its wavefront has).  RESTORE: steps 1, 3 and 4. */
int amx_dti_last_trips(amx_ctx *ctx, const amx_dti *h, int64_t *out_voxel_trips, int64_t *out_wavefront_trips);
/* the last RESTORE call (zeros for the other methods): out[0] voxels that entered step 3, [1] voxels refitted in step 4, [2] voxels at
 * the trip cap or give-up of step 3, [3] voxels left with fewer than 7 samples outside O; waits for that call */
int amx_dti_last_robust(amx_ctx *ctx, const amx_dti *h, int64_t out[4]);
/* y f64[n_vox][nS] -> dirs f64[n_vox][3]; host buffers (blocking) / device buffers (enqueued on hip_stream) */
int amx_dti_directions(amx_ctx *ctx, const amx_dti *h, const double *y, int64_t n_vox, double *out_dirs);
/* (_f32: float32 signals, the dtype amx_prep_gather_device_f32 leaves them in -- same arithmetic, half the bytes)                */
int amx_dti_directions_device_f32(amx_ctx *ctx, const amx_dti *h, const float *d_y, int64_t n_vox, double *d_dirs, void *hip_stream);
int amx_dti_directions_device(amx_ctx *ctx, const amx_dti *h, const double *d_y, int64_t n_vox,
                              double *d_dirs, void *hip_stream);
/* The same fit, keeping what its eigen-decomposition has besides the principal axis (TensorFit.evals / .fa / .md / .ad / .rd of
 * the reference's TensorModel; not part of the reference's own call, which reads .directions only):
 *   evals   f64[n_vox][3]  eigenvalues of D in descending order, then clipped from below at min_diffusivity -- dipy's
 *                          decompose_tensor as TensorModel calls it, min_diffusivity = 1e-6 / -min(design matrix)
 *   scalars f64[n_vox][4]  of the clipped e1 >= e2 >= e3:  FA = sqrt(1/2 ((e1-e2)^2 + (e2-e3)^2 + (e3-e1)^2) / (e1^2 + e2^2 + e3^2))
 *                          (0 where the denominator is 0), MD = (e1 + e2 + e3) / 3, AD = e1, RD = (e2 + e3) / 2
 * min_diffusivity >= 0.  Any of dirs / evals / scalars may be NULL (the host call needs one of them).  With evals and scalars
 * both NULL the call IS amx_dti_directions*: the same checks (dirs must not be NULL then), the same kernel and launch.  With
 * either present a kernel variant runs that computes the same directions, bit for bit.  Limits, error strings (they keep the
 * amx_dti_directions prefix) and the NLLS counters are amx_dti_directions*'s.
 * Samples that are not numbers: a NaN (and -Inf, and any sample below min_signal) counts as min_signal, as it does for the
 * direction -- max(y, min_signal) is taken with fmax -- so the voxel's outputs are finite.  A +Inf sample makes the tensor NaN:
 * evals and scalars are NaN for that voxel (the clip does not hide it); its direction is what amx_dti_directions* writes.  An
 * all-zero or constant voxel has D = 0 to rounding: evals = min_diffusivity three times, FA = 0, MD = AD = RD = min_diffusivity. */
int amx_dti_fit(amx_ctx *ctx, const amx_dti *h, const double *y, int64_t n_vox, double min_diffusivity, double *out_dirs,
                double *out_evals, double *out_scalars);
int amx_dti_fit_device_f32(amx_ctx *ctx, const amx_dti *h, const float *d_y, int64_t n_vox, double min_diffusivity, double *d_dirs,
                           double *d_evals, double *d_scalars, void *hip_stream);
int amx_dti_fit_device(amx_ctx *ctx, const amx_dti *h, const double *d_y, int64_t n_vox, double min_diffusivity, double *d_dirs,
                       double *d_evals, double *d_scalars, void *hip_stream);
/* amx_dti_fit* of a RESTORE estimator (AMX_E_BADARG for any other), and outliers int32[n_vox] = |O| of step 4 (may be NULL; the host
 * call needs one output).  amx_dti_directions*, amx_dti_fit* and amx_prep_gather_directions_device_f32 take a RESTORE estimator too
 * and are this call without the outlier output.  Odd samples are NLLS's: a NaN or a sample below min_signal counts as min_signal
 * (and may then be an outlier like any sample); a +Inf sample leaves NaN parameters, no outlier and NaN evals and scalars. */
int amx_dti_fit_robust(amx_ctx *ctx, const amx_dti *h, const double *y, int64_t n_vox, double min_diffusivity, double *out_dirs,
                       double *out_evals, double *out_scalars, int32_t *out_outliers);
int amx_dti_fit_robust_device_f32(amx_ctx *ctx, const amx_dti *h, const float *d_y, int64_t n_vox, double min_diffusivity,
                                  double *d_dirs, double *d_evals, double *d_scalars, int32_t *d_outliers, void *hip_stream);
int amx_dti_fit_robust_device(amx_ctx *ctx, const amx_dti *h, const double *d_y, int64_t n_vox, double min_diffusivity,
                              double *d_dirs, double *d_evals, double *d_scalars, int32_t *d_outliers, void *hip_stream);

/* (f2, f3) signal preparation and result scatter, fused around the masked voxel list:
 *   core.py:209-223  mean_b0s = mean(img[..., b0_idx], axis=3); norm_factor = 1 / mean_b0s, 0 where
 *                    mean_b0s <= b0_min_signal * mean(mean_b0s[mean_b0s > 0]);  img[..., i] *= norm_factor
 *   core.py:225-227  doMergeB0: volumes -> [mean of the b0 volumes] + the DWI volumes
 *   core.py:229-252  doDirectionalAverage: volumes -> [mean of the b0s] + the mean of every shell (sorted by b)
 *   core.py:451-452  y = img[mask == 1, :].astype(double); y[y < 0] = 0
 *   core.py:472-498  RESULTS[...] = zeros(float32 volume); RESULTS[...][mask == 1, :] = per-voxel values
 * All arithmetic before the float64 cast is float32 in the reference's operation order (numpy reduces the
 * fancy-indexed volumes sequentially in index order), so `y` is bit-identical to the reference's.
 *
 * A plan holds the geometry: dims = (X, Y, Z); strides = element strides of the float32 image along
 * (x, y, z, volume) -- any layout: C order, or the Fortran order nibabel hands out; rank = int32[X][Y][Z]
 * (host, C order): position of the voxel in the masked list (its row in `y`), -1 outside the mask -- i.e.
 * cumsum(mask == 1) - 1 in C order, which is the order `img[mask == 1, :]` enumerates voxels in.
 * Output volume j of `y` is the float32 mean of the input volumes group_idx[group_ptr[j] .. group_ptr[j+1])
 * (a group of one = plain copy): identity groups, the b0-merge or the shell average.  b0_idx = scheme.b0_idx.
 * overwrite_in_order != 0 reproduces core.py:231-245 literally: the shell averages are written into a VIEW of
 * the first n_out volumes of the image while later groups still read from it, so output j replaces input
 * volume j before group j+1 is averaged (harmless when the b0 volumes come first and the shells are stored in
 * b-value order; otherwise the reference averages already-replaced volumes, and so does this).            */
typedef struct amx_prep amx_prep;
int  amx_prep_create(amx_ctx *ctx, const int64_t dims[3], const int64_t strides[4], int nS,
                     const int32_t *rank, int64_t n_vox, const int32_t *group_ptr,
                     const int32_t *group_idx, int n_out, const int32_t *b0_idx, int n_b0,
                     int overwrite_in_order, amx_prep **out);
void amx_prep_destroy(amx_prep *p);
/* img -> y f64[n_vox][n_out] (+ mean_b0 f32[n_vox] of the masked voxels when normalize != 0 and the pointer is
 * not NULL).  normalize = doNormalizeSignal; b0_threshold = the right-hand side of core.py:217 (0 by default).
 * A plan carries the work counter of its gather kernel: ONE gather of a plan in flight at a time (calls on one stream are).  */
int amx_prep_gather(amx_ctx *ctx, const amx_prep *p, const float *img, int normalize, float b0_threshold,
                    double *out_y, float *out_mean_b0);
/* (_f32: the prepared signals stay float32 -- every value of core.py:209-268 IS a float32, core.py:451-452 only widen them; the
 * amx_*_fit_device_f32 / amx_dti_directions_device_f32 calls read them in place)                                                  */
int amx_prep_gather_device_f32(amx_ctx *ctx, const amx_prep *p, const float *d_img, int normalize, float b0_threshold,
                               float *d_y, float *d_mean_b0, void *hip_stream);
/* Limit: protocols of up to 512 volumes (nS <= 512, the limit of the fits), in every layout and with every grouping; a longer one is
 * refused with AMX_E_BADARG ("scheme too long for the LDS tile (at most 512 volumes)").  The kernel keeps all nS samples of a
 * 64-voxel tile in LDS.  While two such tiles fit 160 KB (up to about 310 volumes; 158 when the groups may not write in place) a
 * workgroup holds two wavefronts with a tile each; above that it holds one (the long route), and groups that may not write in place
 * are made 64 output volumes at a time.  Both routes compute the same float32 operations in the same order.                       */
int amx_prep_gather_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, int normalize,
                           float b0_threshold, double *d_y, float *d_mean_b0, void *hip_stream);
/* The arithmetic that picks the route, without a device: out = {route (0 refused, 1 two tiles per workgroup, 2 long), wavefronts per
 * workgroup, LDS bytes per workgroup, words of one wavefront's tile}.  identity: every output volume is its input volume; direct:
 * identity and the image not interleaved; inplace: no group reads a volume an earlier output replaced, or overwrite_in_order.
 * (Grouped outputs on a planar image whose groups read no earlier output take the streaming kernels, which hold no tile.)          */
int amx_prep_route(int nS, int n_out, int n_b0, int n_gidx, int identity, int direct, int inplace, int64_t out[4]);
/* The same for the NODDI fit: which kernels a fit of n_vox voxels (a batch of a call of call_vox voxels; 0: the call itself) launches on a
 * dictionary of this shape, as amx_lut_upload_noddi builds it, with every switch at its default -- without a device or a context.  path: the
 * launches in the format of amx_last_path.  out: seeds, global tile, gemm K-steps, gemm passes, gemm window, gcert, repair, rescue, rescue tile
 * in LDS, seeds2, gcert2, wide, third, third-pass min_items, seed-2 max_atoms, seed-2 trip-cap increment, LASSO left-overs in the second half,
 * their count array, seed occ2, seed-2 occ2, seed chunk, wavefronts of the lane kernels / of k_nnls_seed<1> / of k_lasso_seed, build of the
 * stage-1 / stage-2 kernel (NoddiBuild, csrc/amx_noddi_route.hpp), stage 2 in Gram space, build of the stage-3 kernel, number of launches,
 * build of the table kernel (NoddiGemm), signal rows per lane of the projection kernels; then per launch {wavefronts per workgroup, LDS bytes, LDS bytes of its re-run pass}.                                                      */
#define AMX_ROUTE_WORDS 96
int amx_noddi_route(int nS, int n_wm, int n_dwi, int ndirs, int is_exvivo, int64_t n_vox, int64_t call_vox, double lambda1, double lambda2,
                    char *path, int cap, int64_t out[AMX_ROUTE_WORDS]);
/* The same for the FreeWater (model 2), SANDI (3) and CylinderZeppelinBall (4) fits (csrc/amx_small_route.hpp): the route of a fit of n_vox
 * voxels on a dictionary of nS volumes and n_atoms atoms, as the model's upload builds it.  flags: the fit's AMX_F_*; f32: the signals are
 * float32 in HBM; switches_mask: bit 0 AMX_WAVE_PER_VOXEL, 1 AMX_NO_REFILL, 2 AMX_SANDI_ATOM_SPACE, 3 AMX_FW_NO_FUSE (0: the product path).
 * note_buf: the launches in the format of amx_last_path; for a shape the fit refuses (out[12] != 0: it returns AMX_E_BADARG before
 * anything is enqueued) a newline and the text of amx_last_error follow.  out: family (SmallFamily), build N, signal rows per lane, projection
 * on the matrix cores, float32 signals widened first, voxels per bucketing chunk (0: no bucketing), per chunk of the second plan (0: none),
 * tables to prepare (SmallTables), voxels in order (no plan, no per-call counters), padded volumes of the CylinderZeppelinBall tables,
 * wavefronts per workgroup, LDS bytes, LDS bytes of the re-run pass, refusal (SmallRefusal), number of launches.                              */
#define AMX_SMALL_ROUTE_WORDS 15
int amx_small_route(int model, int nS, int n_atoms, int ndirs, int64_t n_vox, double lambda1, double lambda2, unsigned flags, int f32,
                    unsigned switches_mask, char *note_buf, int cap, int64_t out[AMX_SMALL_ROUTE_WORDS]);
/* What the plan's last gather launched (read-only): the kernel's name into buf, out = {workgroups, threads per workgroup, LDS bytes} */
int amx_prep_last_launch(const amx_prep *p, char *buf, int cap, int64_t out[3]);
/* The gather with the tensor fit taken along (round 5): y AND the principal directions of core.py:431-436, 456-458 in ONE pass over
 * the image -- lane = voxel contracts log(max(y, min_signal)) with the helper's pseudo-inverse while the voxel's values are in the
 * gather's LDS tile; what amx_prep_gather_device[_f32] followed by amx_dti_directions_device[_f32] computes (y bit-identical, the
 * directions to rounding: the sum over the volumes runs in index order here).  h: amx_dti_create for the plan's n_out volumes.
 * With a WLS / NLLS handle the call is exactly those two kernels, one after the other.                                             */
int amx_prep_gather_directions_device(amx_ctx *ctx, const amx_prep *p, const amx_dti *h, const float *d_img, int normalize,
                                      float b0_threshold, double *d_y, float *d_mean_b0, double *d_dirs, void *hip_stream);
int amx_prep_gather_directions_device_f32(amx_ctx *ctx, const amx_prep *p, const amx_dti *h, const float *d_img, int normalize,
                                          float b0_threshold, float *d_y, float *d_mean_b0, double *d_dirs, void *hip_stream);
/* self.mean_b0s of EVERY voxel (core.py:213), float32 [X][Y][Z] in C order: input of the threshold above */
int amx_prep_mean_b0(amx_ctx *ctx, const amx_prep *p, const float *img, float *out_mean_b0_volume);
int amx_prep_mean_b0_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, float *d_mean_b0_volume,
                            void *hip_stream);
/* values f64[n_vox][n_cols] -> float32 volume [X][Y][Z][n_cols] (C order), zero outside the mask */
int amx_prep_scatter(amx_ctx *ctx, const amx_prep *p, const double *values, int n_cols, float *out_volume);
int amx_prep_scatter_device(amx_ctx *ctx, const amx_prep *p, const double *d_values, int n_cols,
                            float *d_volume, void *hip_stream);
/* FreeWater's corrected DWI, volume form (rows form, arithmetic: amx_freewater_corrected_device): RESULTS['DWI_corrected'] of
 *              core.py:488-498 -> d_volume f32[X][Y][Z][n_out] (C order; n_out = the plan's prepared
 *              volumes = the dictionary's nS; d_y32 / d_xiso rows in the plan's masked order).  A masked voxel of rank r gets
 *              out[j] = (float)(m * yc) with m = (double)d_mean_b0[r], or 1 when d_mean_b0 is NULL (core.py:493-494); the columns listed
 *              in b0_cols (HOST int32[n_b0_cols], at most 128; 0 = none) get (float)((double)y[r][j] * m) instead (doKeepb0Intact,
 *              core.py:495-496); every other voxel gets zeros from this same kernel: each element of the volume is written exactly
 *              once and no memset precedes it. */
int amx_prep_corrected_device(amx_ctx *ctx, const amx_prep *p, const amx_lut *lut, const float *d_y32, const double *d_xiso,
                              const float *d_mean_b0, const int32_t *b0_cols, int n_b0_cols, float *d_volume, void *hip_stream);

/* The predicted signal, volume form (rows form, arithmetic: amx_predict_device) -> d_volume f32[X][Y][Z][n_out] (C order; n_out = the
 *              plan's prepared volumes = the dictionary's nS; d_x / d_dirs rows in the plan's masked order).  A masked voxel of rank r
 *              gets out[s] = (float)(m * y_est[r][s]) with m = (double)d_mean_b0[r], or 1 when d_mean_b0 is NULL; every other voxel
 *              gets zeros from this same kernel: each element of the volume is written exactly once and no memset precedes it. */
int amx_prep_predicted_device(amx_ctx *ctx, const amx_prep *p, const amx_lut *lut, const double *d_x, int64_t x_stride, int64_t x_offset,
                              const double *d_dirs, const float *d_mean_b0, float *d_volume, void *hip_stream);

/* (f0) Rician debias of the raw signal, core.py:201-206 (doDebiasSignal, DWI-SNR) -> preproc.py:23-36 `debiasRician`:
 *     per voxel with mask != 0:  sigma = DWI[ix,iy,iz,b0_idx].mean() / SNR;  E = argmin_E sum_i (S_i - mu(E_i))^2  from E = S,
 *     mu(e) = sigma sqrt(pi/2) L_{1/2}(-e^2 / (2 sigma^2))  (preproc.py:8-12), the mean of a Rician variable of amplitude e;
 *     voxels outside the mask become 0; the result replaces the image before normalisation, b0 merge and shell average.
 * The functional is separable and mu is increasing and convex on e >= 0, mu(0) = |sigma| sqrt(pi/2) (the noise floor): its minimiser
 * is E_i = mu^-1(S_i) for a sample above the floor and E_i = 0 for one at or below it (zero and negative samples included).  These
 * entry points compute THAT minimiser, sample by sample in fp64 (Newton's method, residual |mu(E) - S| of a few ulp of S); the
 * reference's L-BFGS-B run stops on its relative-reduction test 1e-5 .. 1e-3 b0 away from it ("Rician debias").
 * The b0 mean is taken in the samples' own precision and in numpy's summation order (so `S[b0_idx].mean()` on the host gives the same
 * bits; at most 128 b0 volumes), sigma = that mean / snr and everything after it in fp64.  Only sigma^2 enters: a negative b0 mean
 * acts like its absolute value.  A voxel whose b0 mean is exactly 0 (or not finite) has no sigma -- the reference's objective is NaN
 * for every E there -- and keeps its samples as they are; a NaN sample stays NaN.  A sample whose iteration reaches its trip cap (32;
 * a CPU trial of the same arithmetic needed at most 5 evaluations for S up to 1e7 sigma) is written as it stands and counted:
 * amx_debias_last_unconverged.
 * One debias call per ctx in flight at a time (the per-voxel sigma lives in the ctx).
 *
 * rows form:   S f64 | f32 [n][nS] (C order), b0_idx int32[n_b0] (HOST memory in both forms) -> E f64[n][nS]                      */
int amx_debias_rows(amx_ctx *ctx, const double *S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr, double *out_E);
int amx_debias_rows_f32(amx_ctx *ctx, const float *S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr, double *out_E);
int amx_debias_rows_device(amx_ctx *ctx, const double *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr,
                           double *d_E, void *hip_stream);
int amx_debias_rows_device_f32(amx_ctx *ctx, const float *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0, double snr,
                               double *d_E, void *hip_stream);
/* image form, in place: the float32 image of a plan in its own layout; voxels with mask != 0 (preproc.py:29 -- where the fit gathers
 * mask == 1, core.py:451) get float32(E), all others 0.  The reference carries float64 from here on; one rounding to float32 costs
 * 6e-8 relative and lets amx_prep_mean_b0* / amx_prep_gather* read the result unchanged.  mask u8[X][Y][Z] (host, C order) is
 * uploaded into the plan once.  Scheme and b0 list are the plan's; a plan without b0 volumes is refused.                          */
int amx_prep_set_debias_mask(amx_ctx *ctx, amx_prep *p, const uint8_t *mask);
int amx_prep_debias(amx_ctx *ctx, const amx_prep *p, float *img, double snr);
int amx_prep_debias_device(amx_ctx *ctx, const amx_prep *p, float *d_img, double snr, void *hip_stream);
/* samples of the last debias call on this ctx that reached the trip cap; waits for that call (an event recorded behind its kernels: the
 * stream it was enqueued on may be gone by then) */
int amx_debias_last_unconverged(amx_ctx *ctx, int64_t *out);

/* (f0+) The noise level from the spread of the b0 repeats (Evaluation's key doEstimateNoise; no counterpart in the reference, whose
 * debias and robust tensor fit both take a number the user has to bring).  Per voxel, k = n_b0 in 2 .. 128, samples float32 | float64,
 * everything in fp64 and every operation rounded on its own (no fused multiply-add):
 *     x_i   = (double) S[b0_idx[i]]                       i = 0 .. k-1, in b0_idx order
 *     sum   = ((x_0 + x_1) + x_2) + ...                   sequential
 *     m     = sum / k
 *     q     = ((x_0-m)*(x_0-m) + (x_1-m)*(x_1-m)) + ...   sequential, product then add
 *     sd    = sqrt(q / (k-1))
 *     eligible  <=>  every x_i finite  and  m > 0  and  sd > 0  and  sd finite
 *     mean = m, sd = sd, ratio = m / sd   when eligible; otherwise all three NaN
 * Over the voxels, with c eligible voxels, nu = k - 1 and m_nu = 2 gammaincinv(nu / 2, 1 / 2) / nu (the median of a chi-square variable
 * of nu degrees of freedom over its mean), the caller takes SNR = nanmedian(ratio) sqrt(m_nu), sigma = nanmedian(sd) / sqrt(m_nu)
 * (amico_amd/noise.py): the median commutes with monotone maps, so both are median-unbiased under Gaussian noise for every k >= 2.
 * rows form:   S [n][nS] (C order) in device memory, b0_idx int32[n_b0] in HOST memory -> f64[n] each, row by row.
 * image form:  the float32 image of a plan in the plan's own layout (any element strides); scheme and b0 list are the plan's.  It visits
 *              the voxels of plan rank >= 0 (mask == 1, the fit's selection: core.py:451) and writes f64[n_vox] in rank order -- the
 *              order amx_prep_scatter_device takes.  Nothing but the k b0 samples of those voxels is read and the image is not written.
 * Any of the three output pointers may be NULL, at least one must be given.  n_b0 < 2, n_b0 > 128 or an index outside 0 .. nS-1 is
 * AMX_E_BADARG; n == 0 (a plan without masked voxels) is a no-op.  Enqueued on `hip_stream`; waits for nothing.                   */
int amx_noise_b0_rows_device(amx_ctx *ctx, const double *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0,
                             double *d_mean, double *d_sd, double *d_ratio, void *hip_stream);
int amx_noise_b0_rows_device_f32(amx_ctx *ctx, const float *d_S, int64_t n, int nS, const int32_t *b0_idx, int n_b0,
                                 double *d_mean, double *d_sd, double *d_ratio, void *hip_stream);
int amx_prep_noise_b0_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, double *d_mean, double *d_sd, double *d_ratio,
                             void *hip_stream);
/* The exact median of the non-NaN values of d_v f64[n] (device): d_out[0] / d_out[1] = the lower / upper middle order statistic (ranks
 * (c-1)/2 and c/2 of the c non-NaN values; equal for an odd c; numpy's nanmedian is (d_out[0] + d_out[1]) / 2), *d_count = c; all three
 * in device memory.  n == 0 or nothing but NaNs: c = 0 and NaN in both.  +-Inf are ordinary values; -0.0 sorts before +0.0.  A radix
 * select on the order-preserving 64-bit key of the value (sign bit set -> all bits flipped; otherwise the sign bit flipped), eleven
 * bits a pass (six passes): integer counts only, so the result does not depend on the launch shape or on the order of the atomics.  No host round trip
 * between the passes, nothing synchronises; the workspace is the ctx's, a ring of four slots: at most four calls of a ctx in flight on
 * different streams.                                                                                                               */
int amx_nanmedian_device(amx_ctx *ctx, const double *d_v, int64_t n, double *d_out, int64_t *d_count, void *hip_stream);

/* (f0++) The noise level per voxel by Marchenko-Pastur PCA of its local patch (doEstimateNoise = 'MPPCA'; Veraart et al., NeuroImage 2016,
 * with the degrees-of-freedom correction of Cordero-Grande et al. 2019; no counterpart in the reference).  It needs no b0 repeat and uses
 * all nS volumes.  Input: the float32 image of a plan in the plan's layout; patch edge w in {3, 5}, h = (w-1)/2.
 *   cube of a masked centre voxel c:  per axis a of length D_a the voxels s_a .. s_a + w - 1, s_a = clamp(c_a - h, 0, D_a - w) (at the
 *            volume's border the cube shifts inward);
 *   columns: the cube's voxels of plan rank >= 0 (mask == 1), n of them; rows: the m = nS volumes; values float32 widened to fp64; no mean
 *            is removed;
 *   eligible <=> 2 n >= w^3 and all m n samples finite and the rule below finds a p; otherwise every output of the voxel is NaN;
 *   r = min(m, n), q = max(m, n);  G = X X^T (m <= n) or X^T X (m > n), r x r, accumulated in fp64 (the products of two float32 values
 *            are exact in fp64, only the summation rounds);  eigenvalues ascending lambda_0 <= .. <= lambda_{r-1}, l_i = max(lambda_i, 0) / q;
 *   rule:    for p = 0 .. r-1 with S_p = l_0 + .. + l_p:  gamma_p = (p+1) / (q - (r-p-1)),  s1 = S_p / (p+1),
 *            s2 = (l_p - l_0) / (4 sqrt(gamma_p));  whenever s2 < s1: sigma^2 = s1, cut = p + 1 (the last such p wins);
 *            sigma = sqrt(sigma^2), n_signal = r - cut;
 *   mean   = the fp64 mean of the centre voxel's b0 samples with the arithmetic of amx_noise_b0_* above (sequential sum in b0_idx order,
 *            one division); NaN without a b0 volume or with a mean <= 0;  ratio = mean / sigma.
 * The eigenvalues come from a Householder tridiagonalisation and Sturm-count bisection (56 halvings of the Gershgorin interval); every
 * threshold in them is a power-of-two fraction of the matrix' own Gershgorin bound, so the outputs of 2^k img are 2^k times those of
 * img, bit for bit.  Over the image the caller takes sigma_est = nanmedian(sigma), SNR_est = nanmedian(ratio) (amx_nanmedian_device; no
 * chi-square factor: sigma is no sample standard deviation).  On small patches the estimate is a few percent low.
 * Outputs fp64 [n_vox] in the plan's masked order, d_eig fp64 [n_vox][125]: the r eigenvalues ascending, then NaN (it exists for the
 * tests).  Every output is optional, at least one must be given, and they may not overlap.  patch not 3 or 5, nS > 512, an axis shorter
 * than the patch, a plan without masked voxels: AMX_E_BADARG.  Enqueued on `hip_stream`; waits for nothing.                          */
int amx_prep_noise_mppca_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, int patch, double *d_sigma, double *d_nsignal,
                                double *d_mean, double *d_ratio, double *d_eig, void *hip_stream);
/* The arithmetic of that kernel's launch without a device, for a patch of n_cols masked columns in a volume of extents dims:
 * out = {1 (0 and AMX_E_BADARG: refused -- patch not 3 or 5, nS < 1 or > 512, an axis shorter than the patch, n_cols outside 0 .. w^3),
 * r, q, side of the Gram matrix (0: the volumes, G = X X^T; 1: the patch, G = X^T X), its order, samples per staged chunk, wavefronts per
 * patch, patches per workgroup, LDS bytes per workgroup, 2 n_cols >= w^3}.                                                           */
#define AMX_MPPCA_ROUTE_WORDS 10
int amx_mppca_route(int nS, int patch, int n_cols, const int64_t dims[3], int64_t out[AMX_MPPCA_ROUTE_WORDS]);

/* (f0+++) The image denoised by that Marchenko-Pastur PCA (doDenoise = 'MPPCA'; Veraart et al. 2016: the patch's best approximation of
 * rank n_signal, written back to its centre voxel; no overlapping-patch averaging; no counterpart in the reference).  Everything up to
 * and including the rule is (f0++)'s, with the same X (m volumes x n masked columns), r, q, side, ascending lambda and cut;
 * s = n_signal = r - cut.  c = the index of the voxel itself among its cube's masked columns (the cube is clamped at the volume's border:
 * "centre" means the voxel the patch belongs to).  The denoised samples of the voxel are column c of the best rank-s approximation of X:
 *   volumes side (G = X X^T):  x^ = P_s x_c,      P_s = the projector onto the eigenvectors of the s largest eigenvalues of G;
 *   patch side   (G = X^T X):  x^ = X (P_s e_c),  the patch read once more from the image for the product;
 *   s = 0:                     x^ = 0 (the rank-0 reconstruction).
 * With G = Q T Q^T (Q: the Householder reflectors of the tridiagonalisation, kept where G's rows held them) and b = x_c | e_c:
 * b' = Q^T b; for the smaller of the two sets of eigenvalues (the s largest, or the cut smallest) the eigenvectors of T from the bisected
 * eigenvalues by the twisted factorisation (forward pivots d+, backward pivots d-, gamma_i = d+_i + d-_i - (T_ii - lambda), the twist at
 * the smallest |gamma_i|, z from the two recurrences; the pivots kept 2^-104 of the Gershgorin bound away from zero as the Sturm count's
 * are), made orthonormal by Gram-Schmidt, every vector twice against those before it; z' = sum_j u_j (u_j^T b') for the signal set,
 * b' - sum_j u_j (u_j^T b') for the noise set; z = Q z'; x^ = z (volumes side) or X z (patch side), all in fp64.  No absolute constant
 * enters: the outputs of 2^k img are 2^k times those of img, bit for bit.
 * d_out float32, the plan's image layout and extent, required, and no part of d_img (the patches overlap): (float)x^ for a denoised voxel;
 * every other sample -- outside the mask, a voxel that is not eligible -- is copied from d_img by a device copy ahead of the kernel on the
 * same stream.  d_sigma / d_nsignal / d_mean / d_ratio: those of amx_prep_noise_mppca_device, bit for bit.  d_status int32 [n_vox]:
 * 0 denoised, 1 not eligible (passed through), 2 over a route's cap (passed through; no route has a cap today: amx_mppca_denoise_route).
 * d_rows64 fp64 [n_vox][nS]: x^ before the float32 rounding, NaN where status != 0 (it exists for the tests).  All but d_out are optional;
 * no two buffers may overlap.  The refusals are amx_prep_noise_mppca_device's.  Enqueued on `hip_stream`; waits for nothing.         */
int amx_prep_noise_mppca_denoise_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, int patch, float *d_out, double *d_sigma,
                                        double *d_nsignal, double *d_mean, double *d_ratio, int *d_status, double *d_rows64, void *hip_stream);
/* That kernel's launch without a device: out = {1 (0 and AMX_E_BADARG: what amx_mppca_route refuses), r, q, side, wavefronts per patch,
 * patches per workgroup, LDS bytes per patch, LDS bytes per workgroup, eigenvectors of length r the kernel can hold (never fewer than
 * r / 2, the most the smaller set has), the cap on min(s, cut) (0: none), 2 n_cols >= w^3}.                                          */
#define AMX_MPPCA_DENOISE_ROUTE_WORDS 11
int amx_mppca_denoise_route(int nS, int patch, int n_cols, const int64_t dims[3], int64_t out[AMX_MPPCA_DENOISE_ROUTE_WORDS]);

/* (f0+++) Gibbs ringing removed from every slice of the image by local sub-voxel shifts (Kellner, Dhital, Kiselev, Reisert, MRM 2016; no
 * counterpart in the reference; tests/unring_np.py restates this).  A slice is the image at one position of the third spatial axis and one
 * volume, I[n_a][n_b] along (axis_a, axis_b); the mask plays no part.  Constants: M = 20 shifts each way, window 1 .. 3.  Shifts, in this
 * order: s_0 = 0, s_j = j / 40 (j = 1 .. 20), s_(20 + j) = -j / 40 (j = 1 .. 20).
 *   One line f[0 .. n), cyclic (indices mod n):  g_0 = f;  g_j[x] = sum_x' d_j[(x - x') mod n] f[x'],
 *     d_j[t] = (1 / n) sum_kappa cos(2 pi kappa (t + s_j) / n),  kappa = -floor((n - 1) / 2) .. floor((n - 1) / 2) (an even n's Nyquist
 *     term is left out).  Per pixel x and shift j:  TV_L = sum_(t = 1 .. 3) |g_j[x - t] - g_j[x - t - 1]|,
 *     TV_R = sum_(t = 1 .. 3) |g_j[x + t] - g_j[x + t + 1]|.  Of the 82 candidates in the order (0, L), (0, R), (1, L), (1, R), ... the first
 *     strict minimum wins (s = 0 wins every exact tie).  With the winner's s = s_j:  U f[x] = (1 - s) g_j[x] + s g_j[x - 1] for s > 0,
 *     (1 + s) g_j[x] - s g_j[x + 1] otherwise.
 *   One slice:  a_n(k) = 1 + cos(2 pi k / n);  Gx(ka, kb) = a_nb(kb) / (a_na(ka) + a_nb(kb)), 1/2 where the denominator is 0;
 *     Ix = Re IDFT2(DFT2(I) Gx),  Iy = I - Ix;  out = U along axis_a of every line of Ix + U along axis_b of every line of Iy.
 * Everything in fp64 from the float32 samples, one rounding to float32 at the end; the tables in fp64 from integers reduced modulo their
 * period.  No absolute constant enters: the output of 2^k img is 2^k times that of img, bit for bit; it depends on the slice's samples and
 * (n_a, n_b) alone, not on the layout, the axes' positions or the chunk.  A slice that holds a NaN or Inf sample is copied through
 * unchanged, bit for bit, and counted; no other slice is affected.
 * d_img, d_out: float32 images in the plan's geometry and element strides (any layout a plan takes); d_out is required and no part of
 * d_img.  (axis_a, axis_b): two different axes out of 0, 1, 2 of the plan's dims; each in-plane extent must be 8 .. 256, anything else is
 * AMX_E_BADARG.  The call enqueues on `hip_stream`, works through the slices in chunks (amx_unring_route) and waits for the last one:
 * *slices = slices in the image, *passed_through = those copied through (either may be null).  Scratch is the ctx workspace: the tables
 * and one chunk of slices, five fp64 planes each -- never more than AMX_UNRING_SCRATCH_CAP bytes, whatever the number of volumes.       */
#define AMX_UNRING_MIN_EXTENT 8
#define AMX_UNRING_MAX_EXTENT 256
#define AMX_UNRING_SCRATCH_CAP (128ll << 20)
int amx_prep_unring_device(amx_ctx *ctx, const amx_prep *p, const float *d_img, float *d_out, int axis_a, int axis_b, int64_t *slices,
                           int64_t *passed_through, void *hip_stream);
/* What a launch asks for, without a device: out = {1 (0 and AMX_E_BADARG: an extent outside 8 .. 256), tile rows, lines per workgroup, tile
 * depth (the 16 x 16 x 4 fp64 MFMA), n_a and n_b rounded up to the tile, workgroups per slice for the lines along a / along b, LDS bytes
 * per workgroup of k_unring_dft / of k_unring_shift, bytes of the tables (with the 512-byte head), scratch bytes per slice, slices per
 * chunk, AMX_UNRING_SCRATCH_CAP}: tables + chunk * per slice, as the grow-only workspace rounds it up, stays under the cap.          */
#define AMX_UNRING_ROUTE_WORDS 14
int amx_unring_route(int n_a, int n_b, int64_t out[AMX_UNRING_ROUTE_WORDS]);

/* (f0') NaN / Inf samples, load_data(..., replace_bad_voxels): core.py:152-158 on the raw image and core.py:270-276 on the
 * pre-processed one --
 *     if np.isnan(img).any() or np.isinf(img).any():
 *         replace_bad_voxels is None -> ERROR(...);  else np.nan_to_num(img, copy=False, nan=r, posinf=r, neginf=r)
 * These entry points COUNT the non-finite elements of a buffer (every exponent bit set, tested on the integer pattern) and, with
 * replace != 0, overwrite exactly those with `value`: NaN, +Inf and -Inf all become value, every finite element -- -0.0 and denormals
 * included -- keeps its bits, and on clean data the buffer is only read.  With replace == 0 the buffer is only read whatever it holds.
 * replace != 0 with a non-finite value is AMX_E_BADARG.  Refusing or warning is the caller's part (amico_amd.core.Evaluation).
 * flat form:   `count` contiguous float32 | float64 elements in device memory (the prepared signals y), aligned to 4 bytes.
 * image form:  the float32 image of a plan in the plan's own layout, every voxel inside and outside the mask as in the reference.  A
 *              layout that is a permutation of a contiguous block (C order, the Fortran order nibabel hands out) is scanned as that
 *              block; any other view is visited element by element, and memory between its elements is neither counted nor written.
 * The device forms are enqueued on `hip_stream` and wait for nothing.  amx_sanitize_last gives the count of the last sanitize call on
 * this ctx, amx_sanitize_previous that of the call before it (a chain scans the image and then y on one stream and reads both at
 * its end); each waits for its call through an event recorded behind the kernel and gives 0 when there was no such call.  The ctx
 * keeps those two counters: a third call reuses the first one's, so calls on different streams must not leave more than two in flight.
 * An amx_prep_ingest* call (below) takes one of the two counters exactly like a sanitize call: it counts as one of the two in flight,
 * and amx_sanitize_last / amx_sanitize_previous read its count. */
int amx_prep_sanitize(amx_ctx *ctx, const amx_prep *p, float *img, int replace, float value, int64_t *out_count);   /* host image, in place */
int amx_prep_sanitize_device(amx_ctx *ctx, const amx_prep *p, float *d_img, int replace, float value, void *hip_stream);
int amx_sanitize_device_f32(amx_ctx *ctx, float *d_buf, int64_t count, int replace, float value, void *hip_stream);
int amx_sanitize_device(amx_ctx *ctx, double *d_buf, int64_t count, int replace, double value, void *hip_stream);
int amx_sanitize(amx_ctx *ctx, double *buf, int64_t count, int replace, double value, int64_t *out_count);          /* host buffer, in place */
int amx_sanitize_last(amx_ctx *ctx, int64_t *out_count);
int amx_sanitize_previous(amx_ctx *ctx, int64_t *out_count);

/* (f0'') The image in its STORED dtype -> the float32 image, core.py:136 `niiDWI_img = img.astype(np.float32)` in HBM, fused with the
 * scan above: the raw bytes cross the link as they are stored (int16 with scl_slope / scl_inter: half the bytes of float32; the
 * float64 of nibabel's get_fdata() needs no host pass to narrow it), are read once and every float32 element is written once.
 * raw_dtype: one of AMX_T_*.  d_raw has the plan's geometry and the plan's ELEMENT strides -- those of the float32 image, counted in
 * elements of its own type; d_img receives the float32 image in the plan's layout.  The two buffers must not overlap; d_raw is
 * aligned to its element size (a block of 2-byte elements may start at any multiple of 2 bytes), d_img to 4 bytes.
 * Value rule -- the reference is numpy:
 *     slope == 1 && inter == 0:   out = np.float32(raw)       round to nearest even from int32 and float64; float64 beyond float32's range
 *                                                             -> +-Inf; denormals and -0.0 are preserved; NaN stays NaN; float32 keeps its bits
 *     otherwise:                  out = np.float32(np.float64(raw) * slope + inter)       product and sum each rounded in fp64 (no fused
 *                                                             multiply-add), as nibabel scales and core.py:136 then narrows
 * slope and inter must be finite (AMX_E_BADARG).  The same kernel counts the non-finite float32 RESULTS (integer pattern; NaN, +Inf, -Inf)
 * and with replace != 0 stores `value` in their place, exactly what amx_prep_sanitize_device does on that float32 image; a non-finite
 * value with replace != 0 is AMX_E_BADARG.  The count is read through amx_sanitize_last / amx_sanitize_previous (see above).
 * Layout: a plan whose image is a permutation of a contiguous block (C order, nibabel's Fortran order) is streamed as that block,
 * every element inside and outside the mask.  Any other view is refused (AMX_E_BADARG, message in amx_last_error): its caller converts
 * on the host and takes amx_prep_sanitize_device.  The device form is enqueued on `hip_stream` and waits for nothing; the host form
 * uploads `raw`, converts, writes the float32 image to `img` and returns the count (blocking). */
#define AMX_T_U8   1
#define AMX_T_I16  2
#define AMX_T_U16  3
#define AMX_T_I32  4
#define AMX_T_F32  5
#define AMX_T_F64  6
int amx_prep_ingest_device(amx_ctx *ctx, const amx_prep *p, const void *d_raw, int raw_dtype, double slope, double inter, int replace,
                           float value, float *d_img, void *hip_stream);
int amx_prep_ingest(amx_ctx *ctx, const amx_prep *p, const void *raw, int raw_dtype, double slope, double inter, int replace, float value,
                    float *img, int64_t *out_count);

/* (f4) LUT resampling to the subject's scheme, lut.pyx:274-311 `resample_kernel` (called per atom by
 * NODDI.resample models.pyx:754-792, FreeWater.resample :1113-1144, ...):
 *     KR = np.ones((ndirs, nS), float32);  KR[i, idx_out] = np.dot(Ylm_out, KRlm[i, :])   for i in range(ndirs)
 * batched over all atoms: lm f32[n_rows][n_sh] = the rotated SH coefficients of n_rows = atoms * ndirs
 * (atom, orientation) pairs (an isotropic atom is one row), ylm_out f32[n_out][n_sh] and idx_out int32[n_out]
 * from aux_structures_resample (lut.pyx:196-224); out f32[n_rows][nS] (host).  One float32 GEMM on the matrix
 * cores; sums are ordered differently from the reference's BLAS sgemv (float32 rounding, ~1e-6 relative).     */
int amx_lut_resample(amx_ctx *ctx, const float *lm, int64_t n_rows, int n_sh, const float *ylm_out,
                     const int32_t *idx_out, int n_out, int nS, float *out);

/* (f4 tail) lut.pyx:227-271 `rotate_kernel` fused with the resampling above, for all anisotropic atoms of a model:
 *     KRlm[i, idx_OUT[s]] = AUX['const'] * Klm[s][AUX['idx_m0']] * AUX['Ylm_rot'][i]        (addition theorem, :262-264)
 * is never materialised (ndirs x nSH x shells floats per atom: 52 MB for NODDI) -- the GEMM forms its left operand in
 * registers from  zonal f32[n_atoms][n_shells * n_sh_shell] = const * Klm[s][idx_m0]  (host, a few KB per atom: the SH
 * fit of the z-aligned response function) and  ylm_rot f32[ndirs][n_sh_shell] = AUX['Ylm_rot'];
 * out f32[n_atoms][ndirs][nS] = what resample_kernel returns for rotate_kernel's output.                          */
int amx_lut_rotate_resample(amx_ctx *ctx, const float *zonal, int n_atoms, const float *ylm_rot, int ndirs,
                            int n_sh_shell, int n_shells, const float *ylm_out, const int32_t *idx_out, int n_out,
                            int nS, float *out);

/* Which of the GEMM's three kernels a shape gets, without a device (the arithmetic both calls above launch by, csrc/amx_lut_route.hpp):
 * n_sh = K reduction indices (for the fused call n_sh_shell * n_shells), n_out DWI volumes, fused = 1 for amx_lut_rotate_resample.
 * out = {route (0 refused: a fused shape beyond K <= 256 / an operator of 80 KB, AMX_E_BADARG from the call; 1 tile: both operands in
 * LDS, plain input with K in 88 90 92 180 182 184 252 254 256 while operator + four row tiles fit 160 KB; 2 lds: the operator in at
 * most 80 KB of LDS, K <= 256, the only fused kernel; 3 generic: operands from L2), compile-time half-length 23 / 46 / 64, dynamic LDS
 * bytes per workgroup}.                                                                                                              */
int amx_lut_route(int n_sh, int n_out, int fused, int64_t out[3]);

/* ---- measurement hooks (bench.py): HIP-event time of the solver kernels of the LAST
 * *_fit_device call on this ctx, measured on the stream they were launched on.
 * which: 0 = all kernels of the call, 1..3 = solver stage kernels (NODDI: the wavefront-per-voxel kernels of NNLS-1, LASSO,
 * NNLS-3 incl. their re-run kernels -- with seeds on they see only the voxels the Gram-space certificates left over;
 * FreeWater/SANDI: 1 = the single solver kernel), 4 = the last amx_dti_directions_device / amx_prep_gather_device kernel,
 * 5..7 = NODDI kernels ahead of stage 1 / 2 / 3 (A'y on the matrix cores + seed solver + Gram-space certificate,
 * csrc/amx_seed.hpp; an error if seeds are off), 8 = k_nnls_seed<1> alone, 9 = k_lasso_seed alone.
 * Requires amx_set_profiling(1) -- or amx_set_profiling(2 + which): only that pair of events is recorded (every recorded event is a
 * packet of the stream, ~5 us of the call: the full set costs a NODDI fit ~70 us, which is why profiling is off by default). */
int amx_set_profiling(amx_ctx *ctx, int enable);
int amx_last_kernel_ms(amx_ctx *ctx, int which, float *out_ms);
/* solver statistics of the last call: out[0]=voxels re-run with the large active-set
 * variant (stage sum), out[1]=voxels hitting the iteration cap, out[2..3] reserved        */
int amx_last_stats(amx_ctx *ctx, int64_t out[4]);
/* NODDI, the seed -> certificate chain (csrc/amx_seed.hpp; no counterpart in the reference, whose every voxel takes one path,
 * models.pyx:902-981): how the voxels fitted since the previous amx_sync_status were settled.  out[0] = voxels that took the
 * chain (0: the calls were too small / the dictionary has no bases), out[1..3] = voxels the Gram-space certificates of stage 1 /
 * the LASSO stage / stage 3 could NOT settle and handed to the wavefront-per-voxel kernels, out[4] = voxels whose stage-2 signal
 * y2 = max(0, y - x_iso iso) was clipped (models.pyx:924-925), out[5..7] reserved.  Certification rate of stage k = 1 - out[k] / out[0]. */
int amx_last_seed_stats(amx_ctx *ctx, int64_t out[8]);
/* Host-buffer entry points, float64 signals: evaluation.y is the float64 cast of a float32 image (core.py:136, 209-223, 451), so its
 * values cross PCIe as float32 -- host threads narrow slices into pinned slots and CHECK every element; one value that is not a
 * float32 (or a NaN) and that batch and the rest of the call are copied as they are (csrc/amx_stage.hpp).  The kernels read the
 * caller's values bit for bit either way.  Returns the number of batches of the LAST host-buffer call that travelled as float32
 * (0: small call, not float32 data, AMX_HOST_NARROW=0, or a *_f32 call -- those are float32 already).  No counterpart in the
 * reference (its fit reads host memory in place, models.pyx:902).                                                              */
int amx_last_host_narrowed(amx_ctx *ctx);

/* The host threads of the float32 transport above (made at the first large float64 host-buffer call of the ctx): out[0] = threads, out[1] =
 * first CPU and out[2] = number of physical cores of the share of the device's NUMA node they are striped over, out[3] = the device.  A
 * node's cores are divided among the devices that hang on it (one pool per device, whether one process drives them all --
 * amico_amd.models: AMX_DEVICES -- or one process each), so that sibling pools never share a core; AMX_HOST_SIBLINGS="i/n" forces the share. */
int amx_host_pool_info(amx_ctx *ctx, int out[4]);
/* The kernels the LAST *_fit / *_fit_device call on this ctx enqueued, in launch order, as text ("k_noddi_gemm<false,25,9> -> k_nnls_seed<1,8,occ2>
 * -> ..."; the first batch of a host-buffer call): which of the library's paths a dictionary shape / call size / solver parameters took.
 * bench.py labels its roofline kernel from it instead of from a literal.  No counterpart in the reference (one path, models.pyx:902-981). */
int amx_last_path(amx_ctx *ctx, char *buf, int cap);

/* device self-test of the wavefront primitives (DPP reductions, broadcasts): writes 12 rows of
 * 64 doubles (sum, max, min, bcast lane 37, next-lane, popcount(ballot v>0), int bcast, v, and
 * the four batched sums of wave_sum4) */
int amx_selftest(amx_ctx *ctx, double *out768);

#ifdef __cplusplus
}
#endif
#endif /* AMICO_AMD_H */
