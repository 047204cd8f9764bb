// amx_small_route.hpp -- which kernels a FreeWater, SANDI or CylinderZeppelinBall fit launches, in which build, with how many wavefronts and
// how much LDS, as plain arithmetic (no HIP in here): amx_fit_dev computes the route once per fit, the model's fit, its amx_*_prepare and
// every amx_launch_* follow it and decide nothing; amx_small_route hands it out, so a test without a GPU can walk every shape
// (tests/test_small_route.py).  DESIGN.md section 14 has the tables.
#pragma once
#include "../../include/amico_amd.h"      // the AMX_F_* flags
#include "amx_sizes.hpp"

namespace amx {

// ------------------------------------------------------------------ thresholds
constexpr int kSmallMaxAtoms = 64;     // what the wavefront-per-voxel kernels of these models hold (a lane per atom); beyond: k_enet_big
constexpr int kBigMaxAtoms = 256;      // ... a thread per atom
constexpr int kLaneMaxAtoms = 16;      // the lane-per-voxel kernels' largest build
// lane-per-voxel solvers work on H = A'A + lambda2 I (Gram space): they need the ridge to bound cond(H); with lambda2 (nearly) 0 the
// problem goes to the QR solver in A-space (wavefront per voxel), like the reference's lasso, which accepts any lambda2 >= 0
constexpr double kLaneMinLam2 = 1e-9;
// (amx_warm_start, amx_sizes.hpp: the projection + block-pivoting kernels -- fused, refill, k_sandi_rows -- assume the warm start: with
//  lambda2 < 1e-5 the fit goes to the Lawson-Hanson lane kernels -- single exchanges from the empty set, which is all block pivoting could
//  do there, ran into the iteration cap on 15 % of the voxels at lambda2 = 1e-6)
constexpr int kFwRefillMaxAtoms = 12;  // FreeWater with lanes that never idle (k_freewater_fused / k_freewater_refill): the reference's 11 (Human) and 12 (Mouse)
constexpr int kFwFuseMinNS = 64;       // k_freewater_fused's pipeline: four or more full tiles of 16 values per voxel, dictionary operand in registers
// The refill gate: k_fw_project's LDS at 12 atoms and 4 wavefronts, two workgroups per CU.  The gate has always counted a 12 x 64 block per
// wavefront that the kernel does not allocate, and 16 spare bytes: they stay in the gate, because it is what sends 228 .. 484 volumes to
// k_freewater_lane, and moving a shape to another kernel is not this header's business.
constexpr size_t kFwRefillGateExtra = (size_t)4 * 12 * 64 * sizeof(double) + 16;
constexpr int kSandiShortNS = 128;     // up to here a wavefront's lanes hold the signal rows (k_sandi<2>) / a lane walks its own row (k_sandi_lane); beyond: amx_sandi_long.hip
constexpr int kSandiRowsNS = 6, kSandiRowsAtoms = 15;      // the default protocol after the directional average: k_sandi_rows<6,15>
// CylinderZeppelinBall's fast route (amx_czb.hip): strong ridge (models.pyx:439 default: 4.0), maps only, one voxel per lane holds <= 32 atoms
constexpr int kCzbFastMaxAtoms = 32, kCzbShortNS = 100, kCzbFastMaxNS = 160;      // k_czb_project<25> / <40>: 25 / 40 K-steps of 4 samples
constexpr double kCzbFastMinLam2 = 1e-2;
constexpr double kCzbGramMinLam2 = 1e-6;                   // below: thin QR in A-space (k_czb_qr)
constexpr int kCzbLdG = 64;            // row stride of the Gram matrices amx_lut_upload_czb builds for <= 64 atoms
constexpr int kCzbBlocksChunk = 2048;  // voxels per chunk of the fast route's second plan
constexpr int czb_padded_nS(int nS) { return nS <= kCzbShortNS ? kCzbShortNS : kCzbFastMaxNS; }
// SANDI, long protocols: K-steps of the A' operand of one atom tile (k_sandi_project), atoms padded to MFMA tiles
constexpr int sl_ksteps(int nS) { return 4 * ((nS + 15) / 16); }
constexpr int sl_padded_atoms(int n_atoms) { return ((n_atoms + 15) / 16) * 16; }

// voxels of one orientation per workgroup of FreeWater's refill kernels: large enough to keep the lanes fed (the buffer needs a
// pool to draw from), small enough for ~3 rounds of workgroups over the chip (measured on 2 M voxels: 512 -> 1.83 ms,
// 1024 -> 1.79, 2048 -> 1.93, 4096 -> 2.54)
constexpr int amx_refill_chunk(long long n_vox)
{
    const long long c = n_vox / 1536;
    return (int)(c < 512 ? 512 : (c > 2048 ? 2048 : c));
}

// ------------------------------------------------------------------ inputs
struct SmallShape {
    int model, nS, ldA, n_atoms, ndirs;      // model: 2 FreeWater, 3 SANDI, 4 CylinderZeppelinBall
    bool has_gram;                           // CylinderZeppelinBall, and every dictionary of more than kSmallMaxAtoms atoms
};
struct SmallCall {
    long long n;
    double lam1, lam2;
    unsigned flags;
    bool f32;                                // the signals are float32 in HBM
};
struct SmallSwitches { bool wave_per_voxel, no_refill, sandi_atom_space, fw_no_fuse; };      // amx_ctx::opt_* (kSwitches)

// ------------------------------------------------------------------ the route
enum SmallFamily {
    SF_NONE = 0,
    SF_FW_FUSED, SF_FW_REFILL,               // FreeWater: k_freewater_fused<N>; k_fw_project[_mfma]<N> + k_freewater_refill<N>
    SF_LANE, SF_WAVE,                        // FreeWater, SANDI: k_*_lane<N>; k_freewater / k_sandi, NR rows per lane
    SF_SANDI_ROWS,                           // k_sandi_rows<6,15>
    SF_SANDI_LONG_LANE, SF_SANDI_LONG_WAVE,  // k_sandi_project + k_sandi_gram_lane<N> / k_sandi_gram_wave
    SF_CZB_FAST, SF_CZB_GRAM, SF_CZB_QR,     // k_czb_project<N> + k_czb_lane (+ k_czb<NR> on its overflow list); k_czb<NR>; k_czb_qr<NR>
    SF_ENET_BIG                              // more than kSmallMaxAtoms atoms, any model
};
enum SmallTables { SMT_NONE = 0, SMT_FW, SMT_SANDI, SMT_SANDI_LONG, SMT_CZB };      // the per-dictionary tables the fit needs prepared (amx_*_prepare)
enum SmallRefusal { SMR_NONE = 0, SMR_SANDI_LONG_RIDGE, SMR_PAIR_TILE, SMR_LANE_TILE, SMR_SANDI_LONG_OPERAND, SMR_BIG_NO_GRAM, SMR_BIG_VECTORS };
constexpr const char *kSmallRefusal[] = {
    "",
    // protocols without the directional average need the ridge: an isotropic dictionary has rank <= shells + 1 < n_atoms, so without it the
    // optimum is not unique and A'A alone is singular
    "amx_sandi_fit: protocols of more than 128 volumes need lambda2 >= 1e-9 (Gram-space solver)",
    "dictionary tile does not fit the 160 KB LDS of a CU (nS x n_atoms too large)",
    "dictionary tile does not fit the 160 KB LDS of a CU",
    "k_sandi_project: the A' operand of one atom tile does not fit the 160 KB LDS of a CU",
    "k_enet_big: the dictionary has no Gram table",
    "k_enet_big: the dictionary's vectors do not fit the LDS"};

struct SmallRoute {
    int family;                  // SmallFamily
    int N;                       // the build: atoms of a lane kernel's template (11 / 12 / 15 / 16), K-steps of k_czb_project (25 / 40); 0: none
    int NR;                      // signal rows per lane of the wavefront-per-voxel kernel (SF_CZB_FAST: of the one behind k_czb_lane's overflow list)
    bool mfma;                   // SF_FW_REFILL: the projection runs on the matrix cores (k_fw_project_mfma)
    bool widen;                  // float32 signals get a float64 copy first (k_widen): the route's kernels read float64 only
    int chunk, blocks_chunk;     // voxels per chunk of the bucketing (kChunk / amx_refill_chunk), of the second plan (0: none)
    int tables;                  // SmallTables
    bool in_order;               // the voxels in order (SANDI has one dictionary): no plan, counts straight into the status words, no per-call counters
    int nSp;                     // SF_CZB_FAST: volumes padded to the projection's K-steps
    int waves;                   // wavefront-per-voxel kernels: wavefronts per workgroup of the main pass, after halving until it fits
    size_t lds, lds_list;        // LDS of the main pass (SF_LANE: of its one pass, SF_SANDI_LONG_*: of k_sandi_project) and of the one-wavefront
                                 // re-run pass; 0: static LDS, or a layout private to the kernel's own unit (fused, refill, k_czb_lane)
    int refusal;                 // SmallRefusal: the fit returns AMX_E_BADARG with `error` before anything is enqueued
    const char *error;
    const char *launch[3]; int n_launch;      // what amx_note records, in launch order (a refused fit: what it had recorded when it was refused)
};

// a wavefront-per-voxel kernel pair: `full` wavefronts at most, halved until the main pass fits; extra: LDS of the main pass beside fit_lds_bytes
inline void small_wave_kernel(SmallRoute &r, const SmallShape &sh, size_t elem, int full, int MP, int MB, bool gram, size_t extra)
{
    r.waves = full;
    while (r.waves > 1 && fit_lds_bytes(elem, sh.nS, sh.ldA, r.NR, 1, r.waves, MP, gram) + extra > kLdsPerCU) r.waves >>= 1;
    r.lds = fit_lds_bytes(elem, sh.nS, sh.ldA, r.NR, 1, r.waves, MP, gram) + extra;
    r.lds_list = fit_lds_bytes(elem, sh.nS, sh.ldA, r.NR, 1, 1, MB, gram);
    if (r.lds > kLdsPerCU || r.lds_list > kLdsPerCU) { r.refusal = SMR_PAIR_TILE; r.error = kSmallRefusal[SMR_PAIR_TILE]; }      // (its kernel is noted by then)
}

inline SmallRoute small_route(const SmallShape &sh, const SmallCall &c, const SmallSwitches &sw)
{
    SmallRoute r{};
    auto note = [&](const char *what) { r.launch[r.n_launch++] = what; };
    auto refuse = [&](int why) { r.refusal = why; r.error = kSmallRefusal[why]; return r; };
    const bool fw = sh.model == 2, sandi = sh.model == 3;
    const size_t elem = sandi ? sizeof(double) : sizeof(float);      // SANDI's one tile is float64
    const bool lane = sh.n_atoms <= kLaneMaxAtoms && c.lam2 >= kLaneMinLam2 && !sw.wave_per_voxel;
    const bool warm = amx_warm_start(c.lam2, c.flags);
    const bool errors = (c.flags & (AMX_F_RMSE | AMX_F_NRMSE)) != 0;
    r.chunk = sandi ? 0 : kChunk;            // (SANDI has one dictionary: nothing to bucket)
    r.error = "";
    if (sandi && sh.nS > kSandiShortNS && c.lam2 < kLaneMinLam2) return refuse(SMR_SANDI_LONG_RIDGE);
    // ---- more than 64 atoms: the dense route, whatever the rest (amx_enet_big.hip; SANDI: the voxels in order)
    if (sh.n_atoms > kSmallMaxAtoms) {
        r.family = SF_ENET_BIG; r.in_order = sandi;
        if (!sh.has_gram || sh.n_atoms > kBigMaxAtoms) return refuse(SMR_BIG_NO_GRAM);
        if (bpp::vec_bytes(sh.nS, sh.n_atoms) > kLdsPerCU) return refuse(SMR_BIG_VECTORS);
        note(fw ? "k_enet_big<FreeWater> (65 .. 256 atoms)" : (sandi ? "k_enet_big<SANDI> (65 .. 256 atoms)" : "k_enet_big<CylinderZeppelinBall> (65 .. 256 atoms)"));
        return r;
    }
    // ---- SANDI on protocols without the directional average: c = A'y on the matrix cores (reads float32 or float64), then a Gram-space solver
    if (sandi && sh.nS > kSandiShortNS) {
        r.family = lane ? SF_SANDI_LONG_LANE : SF_SANDI_LONG_WAVE; r.in_order = true; r.tables = SMT_SANDI_LONG;
        r.N = !lane ? 0 : (sh.n_atoms <= 12 ? 12 : (sh.n_atoms <= 15 ? 15 : 16));
        r.lds = (size_t)sl_ksteps(sh.nS) * 64 * sizeof(double);
        if (r.lds > kLdsPerCU) return refuse(SMR_SANDI_LONG_OPERAND);
        note(c.f32 ? "k_sandi_project<float>" : "k_sandi_project<double>");
        note(!lane ? "k_sandi_gram_wave" : (r.N == 12 ? "k_sandi_gram_lane<12>" : (r.N == 15 ? "k_sandi_gram_lane<15>" : "k_sandi_gram_lane<16>")));
        return r;
    }
    // ---- CylinderZeppelinBall: every kernel reads float32 signals in place
    if (!fw && !sandi) {
        // the default problem (strong ridge, <= 32 atoms, maps only): complementary form, one voxel per lane
        if (sh.n_atoms <= kCzbFastMaxAtoms && c.lam2 >= kCzbFastMinLam2 && !errors && !sw.wave_per_voxel && sh.nS <= kCzbFastMaxNS && sh.has_gram) {
            r.family = SF_CZB_FAST; r.tables = SMT_CZB; r.blocks_chunk = kCzbBlocksChunk;
            r.nSp = czb_padded_nS(sh.nS); r.N = r.nSp / 4;
            r.NR = sh.nS <= 128 ? 2 : 4;
            r.lds_list = fit_lds_bytes(elem, sh.nS, sh.ldA, r.NR, 1, 1, 64, true);
            note(r.N == 25 ? "k_czb_project<25>" : "k_czb_project<40>");
            note("k_czb_lane");
            return r;
        }
        // (8 rows per lane: protocols of up to 512 volumes -- the <= 64-atom tile still fits the LDS: 512 x 65 float32 = 133 KB)
        r.NR = sh.nS <= 128 ? 2 : (sh.nS <= 256 ? 4 : 8);
        if (c.lam2 < kCzbGramMinLam2) {          // below what the Gram form can take: thin QR in A-space
            r.family = SF_CZB_QR;
            note(r.NR == 2 ? "k_czb_qr<2>" : (r.NR == 4 ? "k_czb_qr<4>" : "k_czb_qr<8>"));
            small_wave_kernel(r, sh, elem, 4, 32, 64, false, 0);
        } else {                                 // 26 atoms by default: the main kernel's passive set (32) holds them all; G and a second triangle in LDS
            r.family = SF_CZB_GRAM;
            note(r.NR == 2 ? "k_czb<2>" : (r.NR == 4 ? "k_czb<4>" : "k_czb<8>"));
            small_wave_kernel(r, sh, elem, 8, 32, 64, true, ((size_t)sh.n_atoms * kCzbLdG + (size_t)(32 + 1) * (32 + 2) + 32 + 1) * sizeof(double) + 16);
        }
        return r;
    }
    // ---- FreeWater, SANDI (short protocols): wavefront per voxel -- its load_rows reads float32 signals in place
    if (!lane) {
        r.family = SF_WAVE;
        r.NR = fw ? (sh.nS <= 128 ? 2 : (sh.nS <= 256 ? 4 : 8)) : (sh.nS <= 64 ? 1 : 2);
        note(fw ? "k_freewater (wavefront per voxel)" : "k_sandi (wavefront per voxel)");
        small_wave_kernel(r, sh, elem, 8, 16, 64, false, 0);
        return r;
    }
    // ---- one voxel per lane
    if (sandi) {
        // the default protocol after the directional average (b0 + 5 shells = 6 values, 15 atoms): row-space solver on the dictionary's tables
        if (sh.nS == kSandiRowsNS && sh.n_atoms == kSandiRowsAtoms && warm && !sw.sandi_atom_space) {
            r.family = SF_SANDI_ROWS; r.tables = SMT_SANDI; r.in_order = true; r.widen = c.f32;
            note("k_sandi_rows<6,15>");
            return r;
        }
        r.N = sh.n_atoms <= 12 ? 12 : (sh.n_atoms <= 15 ? 15 : 16);
    } else {
        // lanes that never idle: maps only (the error maps / AMX_F_CORRECTED need the signal again and stay with k_freewater_lane;
        // AMX_F_FW_ISO needs only x and selects nothing)
        const bool refill = warm && !sw.no_refill && sh.n_atoms <= kFwRefillMaxAtoms && !errors && !(c.flags & AMX_F_CORRECTED) &&
                            fw_project_lds_bytes(sh.nS, kFwRefillMaxAtoms, 4) + kFwRefillGateExtra <= kLdsPerCU / 2;
        if (refill) {
            // compile-time dictionary sizes: the reference's defaults (11 Human, 12 Mouse) exactly
            r.N = sh.n_atoms <= 11 ? 11 : 12;
            r.tables = SMT_FW; r.chunk = amx_refill_chunk(c.n);
            r.mfma = sh.nS <= 4 * kProjKS;       // ... which is also what reads float32 signals: both fused builds, k_fw_project_mfma<N, true>
            r.widen = c.f32 && !r.mfma;
            if (sh.nS >= kFwFuseMinNS && r.mfma && !sw.fw_no_fuse) {
                r.family = SF_FW_FUSED;
                note(r.N == 11 ? "k_freewater_fused<11>" : "k_freewater_fused<12>");
                return r;
            }
            r.family = SF_FW_REFILL;
            note(r.mfma ? "k_fw_project_mfma" : "k_fw_project");
            note("k_freewater_refill");
            return r;
        }
        r.N = sh.n_atoms <= 11 ? 11 : (sh.n_atoms == 12 ? 12 : 16);
    }
    r.family = SF_LANE; r.widen = c.f32;
    r.lds = lane_lds_bytes(elem, sh.nS, sh.ldA, r.N);
    if (r.lds > kLdsPerCU) return refuse(SMR_LANE_TILE);
    note("lane-per-voxel solver (k_freewater_lane / k_sandi_lane)");
    return r;
}

}  // namespace amx
