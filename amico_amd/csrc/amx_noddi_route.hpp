// amx_noddi_route.hpp -- which build of every kernel a NODDI fit launches, with how many wavefronts and how much LDS, as plain
// arithmetic (no HIP in here): noddi_fit_dev computes the route once per fit and every launcher follows it, amx_noddi_route hands it
// out, so a test without a GPU can walk every shape and call size (tests/test_noddi_route.py).
//
// Two sizes key the thresholds.  call_vox -- the WHOLE call: a host-buffer call's batches, and the shards of amx_set_call_voxels, all take
// the path the whole call asks for, so that they settle the same voxels with the same arithmetic as the one-shot call -- keys the seeded
// chain, both occ2 builds, the third LASSO certificate pass and the rescue pass.  n -- THIS batch -- keys what only sizes work to the
// voxels at hand and changes no result: the seed chunk, the wavefronts of the seed solvers and the small-call builds of the left-over
// kernels (kLeftSmall1, kLeftSmall3: bit-identical maps either way).
#pragma once
#include "amx_sizes.hpp"

namespace amx {

// ------------------------------------------------------------------ thresholds (the switches' defaults: amx_host.hpp, kSwitches)
// calls of fewer voxels run the left-over kernels of stage 1 / stage 3 in their small-call builds (float32 tile, 4 wavefronts, two workgroups per CU).
// Measured (tools/r06/a05.sh; 50 000 / 100 000 / 200 000 / 300 000 / 500 000 / 1 M voxels, fit in ms, round-5 builds 1.441 / 1.817 /
// 2.386 / 2.885 / 4.000 / 6.421): stage 1 alone 1.421 / 1.793 / 2.394 / 2.921 / 4.072 / 6.591; stage 3 alone 1.415 / 1.797 / 2.371 / 2.849 / 3.989 / 6.506
// (its 12-wavefront build spills 117 registers, this one none); the LASSO stage's (two wavefronts, no screening table) lost at every size (1.460 / 1.905 /
// 2.511 / ...) and is gone.  The gain is ~20 us per kernel, not the ~100 the "one round of workgroups instead of two" arithmetic promised: a left-over
// kernel lasts as long as its longest voxel's Lawson-Hanson, whatever the rounds.
constexpr long long kLeftSmall1 = 150000, kLeftSmall3 = 600000;
constexpr long long kRescueFrom = 2000000;   // voxels from which the NNLS certificates run their rescue pass (AMX_RESCUE_FROM)
constexpr long long kThirdFrom = 600000;     // voxels from which protocols of 96 .. 128 stage-2 rows run the third LASSO certificate pass

// per-chunk counts of the lists the chain compacts (Plan::zcount); ZC_CERT2Q: per chunk, what the second LASSO certificate pass leaves that a third could settle
enum { ZC_CERT1 = 0, ZC_RESC1, ZC_CLIP, ZC_CERT2, ZC_CERT2W, ZC_CERT2W3, ZC_CERT3, ZC_RESC3, ZC_CERT2Q, kZCounts };

// ------------------------------------------------------------------ inputs
// which tables amx_lut_upload_noddi builds for a shape: the Gram matrices always; the orientation bases (and with them the LASSO stage's
// basis, screening table and U2'iso) where the scans of the seed solvers and certificates, which hold 160 atoms, can take the dictionary.
// screen2 stands for screen2_S, screen2_kappa0 and u2iso together: amx_build_basis makes the three in one block, and the route sizes the
// LASSO stage's LDS and switches its certificates on by the one flag -- a build that made only some of them would have to split it.
struct NoddiTables { bool basis, gram, gram_dwi, basis2, screen2; };
constexpr int kSeedMaxWm = 144;      // white-matter atoms a seeded LASSO stage holds: nine tiles of 16 in the seed solver's scan
inline NoddiTables noddi_tables(int n_atoms, int n_wm)
{
    const bool basis = n_atoms <= 160 && n_wm <= kSeedMaxWm;
    return {basis, true, true, basis, basis};
}

struct NoddiShape {
    int nS, ldA, n_atoms, n_wm, n_dwi, ndirs, is_exvivo, s2_derive;      // (s2_derive steers an argument of k_s2_prep, no launch)
    NoddiTables has;
};
struct NoddiCall {
    long long n, call_vox;       // this batch, the whole call
    double lam1, lam2;           // (which outputs are asked for -- rmse, nrmse, the modulated maps -- matters to no choice)
};
// the switches that steer a choice (amx_ctx::opt_*, kSwitches)
struct NoddiSwitches {
    bool no_seed, no_gcert, no_gcert_wide, no_screen, no_big_all;
    long long seed_stages, seed_chunk, seed_waves, seed_min_voxels, seed_occ2_from, seed2_occ2_from, rescue_from, gcert_repair, gcert2_third, fork;
};

// ------------------------------------------------------------------ the route
enum NoddiBuild {
    NB_NONE = 0,
    // stages 1 and 3 (tile in LDS): the left-over lists' small-call build, 8 wavefronts on the float32 tile, 12 wavefronts with 12 atoms on the
    // fp64 tile (stage 1), the stage's own wavefront count on the fp64 / on the float32 tile
    NB_SMALL, NB_F32_8, NB_F64_12, NB_F64_NW, NB_F32_NW,
    NB_GLOBAL,                                   // the tile read where it lies (stage 2: Gram space or QR by NoddiKernel::gram)
    NB_GRAM, NB_GRAM_LEFT, NB_QR,                // stage 2, tile in LDS: Gram space (all voxels / the certificates' left-overs), A-space QR
    NB_BIG_ALL                                   // stage 2: straight to k_noddi_lasso_big
};
enum NoddiGemm { NG_NONE = 0, NG_WINDOWS, NG_25_9, NG_25, NG_40 };
constexpr const char *kGemmNote[] = {"", "k_noddi_gemm<windows>", "k_noddi_gemm<false,25,9>", "k_noddi_gemm<false,25>", "k_noddi_gemm<false,40>"};
struct NoddiKernel {
    int build, NR;               // NoddiBuild; signal rows per lane (2 / 4, 8 with the global tile)
    bool gram;                   // stage 2: Gram space (k_noddi<4>; k_noddi_lasso_big behind it)
    int waves;                   // wavefronts per workgroup of the main pass, after halving until it fits
    size_t lds, lds_list;        // LDS of the main pass and of the one-wavefront re-run pass
    const char *note;
};
struct NoddiLaunch { const char *note; int waves; size_t lds, lds_list; };      // (lds 0: static LDS, or sized by the kernel's own unit)
struct NoddiRoute {
    bool seeds;                  // the seed -> certificate chain runs (a dictionary with a basis, a call of at least AMX_SEED_MIN_VOXELS)
    bool global;                 // the wavefront-per-voxel kernels read the tile where it lies (amx_kernels.hpp: GT)
    int NR;                      // signal rows per lane of the projection kernels: 2 / 4 / 8
    int gemm_ks, gemm_n_pass, gemm_win, gemm;      // K-steps (0: no table kernels, seeds certified on the true residual only), windows, NoddiGemm
    size_t gemm_lds1, gemm_lds2;                   // of the stage-1 table and of the clipped voxels' exact pass
    int seed_chunk, max_schunks, seed_waves, seed1_waves, seed2_waves;      // the second plan (make_plan)
    bool seed_occ2, seed2_occ2;
    bool seed1, seed3, gcert, repair, rescue, tile_in_lds;      // stages 1 / 3: seed solver, Gram certificates, their second look, rescue pass (its tile in LDS)
    size_t seed1_lds, seed3_lds, gcert_lds, rescue_lds;
    bool seeds2, gcert2, wide, third;                           // the LASSO stage: seed solver, certificate passes
    int min_items, seed2_max_atoms, seed2_trip_add;
    size_t seed2_lds, gcert2_lds, gcert2_wide_lds;               // (wide: the second and third certificate pass, the chunk's Gram triangle beside the rest)
    bool left2_second_half; int left2_count;                    // where the certificate passes leave their lists: half of ctx->rlist, Plan::zcount
    bool fork1, fork2;           // AMX_FORK
    NoddiKernel s1, s2, s3, s3_fork;      // the stage kernels (s3_fork: AMX_FORK bit 1, stage 3 without seeds on the LASSO left-overs)
    NoddiLaunch launch[20]; int n_launch; // what amx_note records, in launch order
};

// Does this shape run the global-tile variants?  The LDS variants hold <= 256 rows (4 per lane), <= 192 atoms (3 per lane) and need the
// float32 tile + the blocks of at least two wavefronts in LDS (the widest: the LASSO stage's Gram solver with 32 passive atoms; the re-run
// kernels with 64)
inline bool noddi_tile_global(int nS, int ldA, int n_atoms)
{
    if (nS > 256 || n_atoms > 192) return true;
    const int NR = nS <= 128 ? 2 : 4;
    return fit_lds_bytes(4, nS, ldA, NR, 3, 2, 32, true) + kScreenBytes > kLdsPerCU || fit_lds_bytes(4, nS, ldA, NR, 3, 1, 64, true) > kLdsPerCU;
}

// can the table kernels take this dictionary?  (K-steps of 4 samples: 25 or 40 per voxel; one workgroup's operands must fit a CU's LDS)
// (every windowed launch is the KS = 40 build, whatever its window: the LDS size and this fit check must be those of the launched template --
//  161 .. 200 volumes have windows of 84 .. 100 samples and were sized for 25 K-steps until round 6: operands beyond the allocation)
inline int noddi_gemm_ksteps(int nS, int n_atoms, int n_wm)
{
    if (!noddi_tables(n_atoms, n_wm).basis || nS > 512) return 0;
    const int ks = (gemm_passes(nS) > 1 || gemm_window(nS) > 100) ? 40 : 25;
    return gemm_lds(n_atoms, gemm_rows(n_atoms), ks) > kLdsPerCU ? 0 : ks;
}

// one stage kernel: `full` wavefronts at most, halved until the main pass fits (launch_pair does the same and arrives at the same count)
inline NoddiKernel noddi_kernel(int build, int NR, bool gram, const char *note, const NoddiShape &sh, size_t elem, int NQ, int full,
                                int MP, int MB, bool ridge, size_t scr)
{
    const bool gt = build == NB_GLOBAL;
    NoddiKernel k{build, NR, gram, full, 0, 0, note};
    while (k.waves > 1 && fit_lds_bytes(elem, sh.nS, sh.ldA, NR, NQ, k.waves, MP, gram, ridge, gt) + scr > kLdsPerCU) k.waves >>= 1;
    k.lds = fit_lds_bytes(elem, sh.nS, sh.ldA, NR, NQ, k.waves, MP, gram, ridge, gt) + scr;
    k.lds_list = fit_lds_bytes(4, sh.nS, sh.ldA, NR, NQ, 1, MB, gram, ridge, gt);
    return k;
}

// Stages 1 and 3 (NNLS).  left: the kernel walks the lists the Gram certificates left over; scr: the screening table in LDS.
inline NoddiKernel noddi_nnls_kernel(int stage, const NoddiShape &sh, long long n, bool global, bool left, size_t scr)
{
    const char *all = stage == 1 ? "k_noddi<1> (all voxels)" : "k_noddi<3> (all voxels)";
    const char *note = !left ? all : (stage == 1 ? "k_noddi<1> (left-overs of k_nnls_gcert<1>)" : "k_noddi<3> (left-overs)");
    // Any shape the reference's loop takes (models.pyx:825-861: any nS, any n_wm): protocols of more than 256 volumes, dictionaries of more
    // than 192 atoms, and tiles that do not fit a CU's LDS (288 x 145 float32 = 167 KB) run the SAME solver with the tile read where it
    // lies (k_noddi<..., GT = true>: 8 rows and 4 atoms per lane: nS <= 512, n_atoms <= 256), room for 12 (stage 3: 8) passive atoms, 4 wavefronts.
    if (global) return noddi_kernel(NB_GLOBAL, 8, false, note, sh, 4, 4, 4, stage == 1 ? 12 : 8, 32, false, scr);
    const int NR = sh.nS <= 128 ? 2 : 4, NQ = 3, MP = 8, MB = 32;
    // wavefronts per workgroup: as many as the register budget of the stage allows (stage 3, measured with the seeded path: 16 wavefronts -> 128
    // VGPRs and 223 spilled registers, 5.9 ms; 12 -> 168 VGPRs, 3.7 ms)
    const int NW = stage == 1 ? 16 : 12;
    // Left-overs of the Gram certificates (seeded chain): few voxels per chunk, and the ones that get here are the hard ones -- stage 1:
    // room for 12 passive atoms and 12 wavefronts (168 VGPRs, 16 spilled, against 128 / 64 with 8 atoms and 16 wavefronts): nothing
    // overflows into the one-wavefront re-run kernel any more (it cost 0.16 ms for five voxels per million), 1 M voxels 0.82 -> 0.65 ms
    const int MPL = stage == 1 ? 12 : MP;
    auto fits = [&](size_t elem, int nw, int mp, int per_cu) { return per_cu * (fit_lds_bytes(elem, sh.nS, sh.ldA, NR, NQ, nw, mp, false, false) + scr) <= kLdsPerCU; };
    // SMALL calls (round 6): a chunk is an orientation, so even a 50 000-voxel call launches ~500 workgroups here, each with a handful of
    // left-over voxels; the build below holds a whole CU's LDS (154 KB: the fp64 tile) -- 500 workgroups on 256 CUs are TWO rounds, each as long
    // as one hard voxel's Lawson-Hanson (~140 us).  With the float32 tile and 4 wavefronts a workgroup takes 77 KB: two per CU, one round.
    // Same arithmetic (the tile's values are widened when read instead of when staged): bit-identical maps.  Keyed on THIS batch's voxels.
    if (left && n < (stage == 1 ? kLeftSmall1 : kLeftSmall3) && fits(4, 4, MPL, 2))
        return noddi_kernel(NB_SMALL, NR, false, stage == 1 ? "k_noddi<1> (left-overs of k_nnls_gcert<1>; small-call build: two workgroups per CU)"
                                                                  : "k_noddi<3> (left-overs; small-call build: two workgroups per CU)", sh, 4, NQ, 4, MPL, MB, false, scr);
    // Protocols of 129 .. 256 volumes (four signal rows per lane; the fp64 tile of 150 x 145 does not fit the LDS): the left-over lists used to
    // fall through to the full build below -- stage 1: 128 registers, 203 of them spilled; stage 3: twelve wavefronts with 697 spilled registers.
    // Eight wavefronts (two per SIMD, 256 registers: no spills) on the float32 tile (round 6)
    if (NR == 4 && left && fits(4, 8, MPL, 1) && !fits(8, 12, MPL, 1))
        return noddi_kernel(NB_F32_8, NR, false, stage == 1 ? "k_noddi<1> (left-overs of k_nnls_gcert<1>; 8 wavefronts, float32 tile)"
                                                                  : "k_noddi<3> (left-overs; 8 wavefronts, float32 tile)", sh, 4, NQ, 8, MPL, MB, false, scr);
    if (stage == 1 && left && fits(8, 12, MPL, 1)) return noddi_kernel(NB_F64_12, NR, false, note, sh, 8, NQ, 12, MPL, MB, false, scr);
    // fp64 tile in LDS when it fits next to the per-wavefront blocks (99 x 145: 115 KB + 16 x 2.3 KB of 160 KB): the
    // fp32 -> fp64 conversions of the tile reads are then paid once per chunk.
    if (fits(8, NW, MP, 1)) return noddi_kernel(NB_F64_NW, NR, false, note, sh, 8, NQ, NW, MP, MB, false, scr);
    return noddi_kernel(NB_F32_NW, NR, false, note, sh, 4, NQ, NW, MP, MB, false, scr);
}

// Stage 2 (the LASSO).  gram: Gram-space solver (needs the Gram matrices and a ridge that bounds cond(H): lambda2 >= 1e-5), else the QR
// solver in A-space, any lambda2 > 0; left: the lists of the LASSO certificates; seeded: the seed solver ran (NoddiArgs::seeds2)
inline NoddiKernel noddi_lasso_kernel(const NoddiShape &sh, const NoddiCall &c, const NoddiSwitches &sw, bool global, bool gram, bool left, bool seeded, size_t scr)
{
    const char *note = left ? "k_noddi<4|2> (left-overs of k_lasso_gcert)" : "k_noddi<4|2> (all voxels)";
    // lambda1 = 0 (a pure ridge: set_solver(lambda1=0, ...)): the optimum holds most of the dictionary -- every voxel would walk Lawson-Hanson
    // to 20, then 64 atoms and overflow twice on its way to the solver that can hold it: straight there (AMX_BIG_ALL=0: the long way, diagnosis)
    if (gram && c.lam1 == 0.0 && !left && sh.n_wm > 64 && !sw.no_big_all)
        return NoddiKernel{NB_BIG_ALL, 0, true, 4, 0, 0, "k_noddi_lasso_big (all voxels: lambda1 = 0)"};
    // shapes beyond the LDS variants: the tile read where it lies; Gram space: passive sets of up to 32 atoms in the main pass, 64 in the
    // re-run pass; A-space QR: 20 and 32 (the factor lives in registers -- 32 x 8 rows per lane is what a wavefront holds)
    if (global) return gram ? noddi_kernel(NB_GLOBAL, 8, true, note, sh, 4, 4, 4, 32, 64, true, scr) : noddi_kernel(NB_GLOBAL, 8, false, note, sh, 4, 4, 4, 20, 32, true, 0);
    const int NR = sh.nS <= 128 ? 2 : 4;
    if (!gram) return noddi_kernel(NB_QR, NR, false, note, sh, 4, 3, 8, 20, 64, true, 0);
    // left-over lists of the Gram certificates: few voxels, mostly seeds of more than 16 atoms -- half the wavefronts with
    // room for 32 atoms each, so that practically nothing is left for the (slow, one wavefront per voxel) re-run kernel
    // (a small-call build as in stage 1 -- two wavefronts with room for 32 atoms each, no screening table, two workgroups per CU -- lost at
    //  every call size, kLeftSmall1, and is gone)
    if (left && seeded) return noddi_kernel(NB_GRAM_LEFT, NR, true, note, sh, 4, 3, 8, 32, 64, true, scr);
    return noddi_kernel(NB_GRAM, NR, true, note, sh, 4, 3, 16, 20, 64, true, scr);
}

// LDS of the LASSO certificates: S rows, column scales, G[.][iso], S in MFMA operand order, a block per wavefront; the wide passes (one
// workgroup per CU) add the packed lower triangle of the orientation's white-matter Gram block, tri(i, j) = i (i + 1) / 2 + j.
// Every shape with a seeded LASSO stage fits -- 144 atoms: 65 040 + 83 520 B of 163 840 -- so the wide passes have this one path.
constexpr size_t gcert2_lds_bytes(int n_wm)
{
    return ((size_t)n_wm * kSeedLd + 2 + 2 * ((n_wm + 1) & ~1) + (size_t)9 * (kSeedKD / 4) * 64 + (size_t)4 * 64 * 16) * sizeof(double);
}
constexpr size_t gcert2_wide_lds_bytes(int n_wm) { return gcert2_lds_bytes(n_wm) + (size_t)n_wm * (n_wm + 1) / 2 * sizeof(double); }
static_assert(gcert2_wide_lds_bytes(kSeedMaxWm) <= kLdsPerCU, "the wide LASSO certificate passes hold the Gram triangle of every seeded shape in LDS");

inline NoddiRoute noddi_route(const NoddiShape &sh, const NoddiCall &c, const NoddiSwitches &sw)
{
    NoddiRoute r{};
    auto note = [&](const char *what, int waves, size_t lds, size_t lds_list = 0) { r.launch[r.n_launch++] = NoddiLaunch{what, waves, lds, lds_list}; };
    auto stage_kernel = [&](const NoddiKernel &k) {
        note(k.note, k.waves, k.lds, k.lds_list);
        // supports of more than 64 atoms (a weak lambda1: the optimum is dense): the slow exact solver, from the re-run kernel's own overflow list
        if (k.gram && k.build != NB_BIG_ALL) note("k_noddi_lasso_big (supports beyond 64 atoms)", 4, 0);
    };
    r.global = noddi_tile_global(sh.nS, sh.ldA, sh.n_atoms);
    r.NR = sh.nS <= 128 ? 2 : (sh.nS <= 256 ? 4 : 8);
    // (the seeded chain of ~16 kernels has a floor of ~1.5 ms: AMX_SEED_MIN_VOXELS, kSwitches)
    r.seeds = sh.has.basis && sh.has.gram && !sw.no_seed && c.call_vox >= sw.seed_min_voxels;
    r.gemm_ks = r.seeds ? noddi_gemm_ksteps(sh.nS, sh.n_atoms, sh.n_wm) : 0;
    r.gemm_n_pass = gemm_passes(sh.nS); r.gemm_win = gemm_window(sh.nS);
    r.gcert = r.seeds && !sw.no_gcert && r.gemm_ks > 0;
    // ---- the second plan: chunks, wavefronts and builds of the lane kernels
    if (r.seeds) {
        // Chunk of the second plan: whole orientations wherever possible (a lane then walks many voxels and the tail of the chunk
        // is a small share), i.e. about twice the mean population -- 4 M voxels, ndirs 500: 4096 -> 103 M voxels/s (every
        // orientation cut in two or three), 8192 -> 83 M, 16384 -> 123 M; never below 4096 (1 M voxels: 2048 -> 72 M, 4096 -> 99 M).
        r.seed_chunk = (int)sw.seed_chunk;
        if (r.seed_chunk <= 0) {
            const long long want = 2 * c.n / (sh.ndirs > 512 ? sh.ndirs : 512);
            r.seed_chunk = (int)(want < 4096 ? 4096 : (want > 65536 ? 65536 : ((want + 63) & ~63LL)));
        }
        r.max_schunks = (int)(c.n / r.seed_chunk) + sh.ndirs + 1;
        r.seed_waves = sw.seed_waves ? (int)sw.seed_waves : 4;
        // (measured, ndirs = 500: 100 000 / 200 000 / 400 000 / 1 M voxels -> stage-1 group 1.11 / 1.55 / 2.31 / 4.66 ms with two
        //  wavefronts per workgroup against 1.33 / 1.80 / 2.39 / 4.14 ms with four; every other lane kernel is best with four)
        r.seed1_waves = sw.seed_waves ? (int)sw.seed_waves : ((double)c.n / (double)r.max_schunks < 640.0 ? 2 : 4);
        // the two-wavefronts-per-SIMD builds of k_nnls_seed<1> / k_lasso_seed (AMX_SEED_OCC2_FROM, kSwitches: throughput bound calls win)
        r.seed_occ2 = c.call_vox >= sw.seed_occ2_from;      // (batches of one host call all take the same build)
        r.seed2_occ2 = c.call_vox >= sw.seed2_occ2_from;
        r.seed2_waves = r.seed1_waves;
        if (!sw.seed_waves) { if (r.seed_occ2) r.seed1_waves = 4; if (r.seed2_occ2) r.seed2_waves = 4; }
    }
    // ---- stage 1: NNLS on all atoms
    bool left1 = false;
    if (r.seeds) {
        if (r.gcert) {
            const int mtf = sh.n_atoms / 16;
            // windows: always the K-steps 40 build (noddi_gemm_ksteps sizes the LDS for it); the default dictionary: unrolled tile loop
            r.gemm = r.gemm_n_pass > 1 ? NG_WINDOWS : (r.gemm_ks == 25 ? (mtf == 9 ? NG_25_9 : NG_25) : NG_40);
            r.gemm_lds1 = gemm_lds(sh.n_atoms, gemm_rows(sh.n_atoms), r.gemm_ks);
            r.gemm_lds2 = gemm_lds(sh.n_wm, gemm_rows(sh.n_atoms), r.gemm_ks);
            note(kGemmNote[r.gemm], 8, r.gemm_lds1);
        }      // (else k_noddi_project<NR>: y~ = U'y alone, no note)
        r.seed1 = (sw.seed_stages & 1) != 0;
        // S for the per-lane gathers + ticket; stage 1 adds S in MFMA operand order (10 x 3 x 64) and a residual block per wavefront;
        // stage 3: the lanes' candidate byte lists
        const size_t seed_lds = (size_t)sh.n_atoms * kSeedLd * sizeof(double) + 64;
        r.seed1_lds = seed_lds + ((size_t)10 * (kSeedKD / 4) * 64 + (size_t)4 * 64 * (kSeedKD + 1)) * sizeof(double);
        r.seed3_lds = seed_lds + (size_t)256 * kSeed3ListRow;
        r.gcert_lds = ((size_t)sh.n_atoms * kSeedLd + 2 + (size_t)10 * (kSeedKD / 4) * 64 + (size_t)4 * 64 * 16) * sizeof(double);
        // a second look at the seeds a lane can mend itself (k_nnls_gcert<.., REPAIR>): where a left-over voxel is expensive and the seeds are
        // wrong more often -- the shapes whose tile is read from L2 (AMX_GCERT_REPAIR=0 / 1 forces)
        r.repair = sw.gcert_repair >= 0 ? sw.gcert_repair != 0 : r.global;
        // The rescue pass (large calls: below ~2 M voxels the launch costs more than the wavefront-per-voxel kernel saves -- 1 M voxels
        // 8.08 -> 8.24 ms with it, 4 M 24.99 -> 24.38): the supports refused for conditioning, corrected with the signal itself.
        // (ex-vivo dictionaries leave 7 % of the voxels instead of 5 and 2.5 % -- the dot atom makes more supports ill-conditioned -- and
        //  gain from 1 M voxels: 108 -> 112 M voxels/s; deciding on the device from the first pass's count was tried: the launch that only
        //  hands the lists on costs every other call 1 %)
        // (batches of one host-buffer call all take the path the whole call's size asks for, as the seed solvers' builds do:
        //  host and device entry points settle the same voxels with the same arithmetic)
        // (shapes whose tile does not fit the LDS -- an HCP-style protocol -- run it at every size: a left-over voxel costs their
        //  wavefront-per-voxel kernels ten times what it costs the LDS variants, and the lane that corrects a support reads 8 atoms, not the tile)
        // (round 6: ... and protocols of more than 128 volumes, whose wavefront-per-voxel kernels hold four signal rows per lane -- a left-over voxel
        //  costs them 37 ns against 14 at 99 volumes: 150 volumes, 1 M voxels 11.23 -> 10.65 ms with the pass, stage-3 left-overs 38 219 -> 6 429;
        //  at 99 - 105 volumes it still loses below 2 M voxels, SNR 50 included: profiles/r06_protocols_ab.txt)
        const long long rescue_from = sw.rescue_from >= 0 ? sw.rescue_from : kRescueFrom;   // (AMX_RESCUE_FROM given: the caller's threshold alone decides)
        r.rescue = c.call_vox >= (sh.is_exvivo ? rescue_from / 4 : rescue_from) || (sh.nS > 128 && sw.rescue_from < 0) || r.global;
        const size_t tile = (size_t)sh.nS * sh.ldA * sizeof(float);
        r.tile_in_lds = r.gcert_lds + tile <= kLdsPerCU;
        r.rescue_lds = r.gcert_lds + (r.tile_in_lds ? tile : 0);
        if (r.seed1) {
            note(r.seed_occ2 ? "k_nnls_seed<1,8,occ2>" : "k_nnls_seed<1,8>", r.seed1_waves, r.seed1_lds);
            if (r.gcert) {
                note(r.repair ? "k_nnls_gcert<1,repair>" : "k_nnls_gcert<1>", r.seed_waves, r.gcert_lds);
                if (r.rescue) note("k_nnls_gcert<1,rescue>", r.seed_waves, r.rescue_lds);
                left1 = true;
            }
        }
    }
    const bool scr_S = r.seeds && !sw.no_screen;
    r.s1 = noddi_nnls_kernel(1, sh, c.n, r.global, left1, (scr_S && r.seed1) ? kScreenBytes : 0);
    stage_kernel(r.s1);
    r.fork1 = (sw.fork & 1) && left1;
    // ---- stage 2: the LASSO on the white-matter atoms.  Its seeds need x_iso: Gram-space solver only (lambda2 >= 1e-5)
    // (lambda1 = 0: a dense optimum -- no seeds to propose, the stage goes to k_noddi_lasso_big)
    r.seeds2 = r.seeds && (sw.seed_stages & 4) && sh.has.basis2 && c.lam2 >= 1e-5 && (r.gemm_ks > 0 || sh.nS <= 128) &&
               (c.lam1 > 0.0 || sw.no_big_all || sh.n_wm <= 64);
    r.seed2_max_atoms = 20;
    if (r.seeds2) {
        r.gcert2 = !sw.no_gcert && r.gemm_ks > 0 && sh.has.screen2;
        r.wide = r.gcert2 && !sw.no_gcert_wide;
        // A third pass (supports of 19 .. 24 atoms, the triangle mostly in scratch) pays where a left-over voxel is expensive: shapes whose
        // wavefront-per-voxel kernels read their tile from L2 (a 288-volume protocol leaves 6.8 % of the voxels after two passes: 6.5 of that
        // fit's 24 ms went to k_noddi<4, .., GT>).  At 99 volumes it is a wash (round 3: 10.34 against 10.33 ms).  AMX_GCERT2_THIRD=0 / 1 forces.
        // Round 6: the pass is launched for EVERY shape and decides per chunk (Gcert2Args::min_items): a chunk that still holds a block's worth of
        // such supports is worth its tables, one that holds a dozen is handed on as it is.  AMX_GCERT2_THIRD=0: never (the round-5 default for tiles in
        // LDS), 1: every chunk whatever it holds (the round-5 behaviour for global tiles, still their default).
        // lambda1 is fixed while ||A2'y2|| grows with the number of stage-2 rows: beyond the default protocol's 90 the LASSO supports are denser (105
        // volumes = 100 rows: 41 000 of 1 M voxels beyond 18 atoms, against 6 300) -- there the pass runs too, and decides per chunk.
        // (... from kThirdFrom voxels: the pass's kernel holds its 24 x 24 triangle mostly in scratch (2.6 KB per lane) and a block costs it ~0.4 ms whatever
        //  the call's size -- 105 volumes, tools/r06/a12.sh: 300 000 voxels 3.58 ms without, 3.70 with it (0.50 ms of certificates to save 0.38 of
        //  left-over kernel); 1 M voxels 8.59 -> 8.01 (0.72 to save 1.27))
        // (... and up to 128 volumes: at 150 the pass costs 0.5 ms of certificates to save 0.13 of left-over kernel -- most of what is left there holds
        //  more than 24 atoms, or fails for other reasons)
        if (r.wide) r.third = sw.gcert2_third >= 0 ? sw.gcert2_third != 0 : (r.global || (sh.n_dwi > 95 && sh.nS <= 128 && c.call_vox >= kThirdFrom));
        r.min_items = (sw.gcert2_third == 1 || r.global) ? 0 : 16;      // list entries a chunk must hold for the third pass to work on it (16: tiles in LDS)
        // supports of up to 24 atoms are certified lane-per-voxel where the third pass runs: the seed solver goes on to 26 atoms there
        // (and gets 2 atoms per trip: the trip cap grows with it); elsewhere 20 (the second pass ends at 18)
        if (r.third) { r.seed2_max_atoms = 26; r.seed2_trip_add = 6; }
        r.left2_second_half = r.wide && !r.third;      // (an even number of passes after the first ends in the first half again)
        r.left2_count = !r.wide ? ZC_CERT2 : (r.third ? ZC_CERT2W3 : ZC_CERT2W);
        r.seed2_lds = ((size_t)sh.n_wm * (kSeed2KD + 1) + 8 + (size_t)9 * (kSeed2KD / 4) * 64 + (size_t)4 * (64 * (kSeed2KD + 1) + 64 * 3)) * sizeof(double);
        r.gcert2_lds = gcert2_lds_bytes(sh.n_wm);
        r.gcert2_wide_lds = r.wide ? gcert2_wide_lds_bytes(sh.n_wm) : 0;      // (seeds2 asks for the basis tables: n_wm <= kSeedMaxWm, noddi_tables)
        if (r.gcert2) { note("k_s2_prep", 4, 0); note("k_noddi_gemm<lasso> (clipped voxels)", 8, r.gemm_lds2); }      // (else k_noddi_project2<NR>, no note)
        note(r.seed2_occ2 ? "k_lasso_seed<occ2>" : "k_lasso_seed", r.seed2_waves, r.seed2_lds);
        if (r.gcert2) note("k_lasso_gcert<11>", r.seed_waves, r.gcert2_lds);
        if (r.wide) note("k_lasso_gcert<18,wide>", r.seed_waves, r.gcert2_wide_lds);
        if (r.third) note("k_lasso_gcert<24,wide,18>", r.seed_waves, r.gcert2_wide_lds);
        // AMX_FORK bit 1: the voxels these certificates left over do not come back to the lane kernels (noddi_fit_dev)
        r.fork2 = r.gcert2 && (sw.fork & 2) && (sw.seed_stages & 2) && r.gcert;
    }
    r.s2 = noddi_lasso_kernel(sh, c, sw, r.global, sh.has.gram_dwi && c.lam2 >= 1e-5, r.gcert2, r.seeds2,
                              (r.seeds2 && !sw.no_screen && sh.has.screen2) ? kScreenBytes : 0);
    stage_kernel(r.s2);
    if (r.fork2) { r.s3_fork = noddi_nnls_kernel(3, sh, c.n, r.global, true, 0); stage_kernel(r.s3_fork); }
    // ---- stage 3: NNLS on the support + iso
    r.seed3 = r.seeds && (sw.seed_stages & 2);
    if (r.seed3) {
        note("k_nnls_seed<3,6>", r.seed_waves, r.seed3_lds);
        if (r.gcert) {
            note(r.repair ? "k_nnls_gcert<3,repair>" : "k_nnls_gcert<3>", r.seed_waves, r.gcert_lds);
            if (r.rescue) note("k_nnls_gcert<3,rescue>", r.seed_waves, r.rescue_lds);
        }
    }
    r.s3 = noddi_nnls_kernel(3, sh, c.n, r.global, r.seed3 && r.gcert, (scr_S && r.seed3) ? kScreenBytes : 0);
    stage_kernel(r.s3);
    return r;
}

}  // namespace amx
