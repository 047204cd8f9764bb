// amx_sizes.hpp -- the sizes kernels and their launchers share, as plain arithmetic (no HIP in here: the kernel headers include it for
// kWave and the table layouts, amx_noddi_route.hpp for the LDS a launch asks for).
// (no __host__ __device__: the compiler of the HIP units takes a constexpr function on either side)
#pragma once
#include <stddef.h>

namespace amx {

// ------------------------------------------------------------------ sizes the kernels and their launchers share
constexpr int kWave = 64;
constexpr size_t kLdsPerCU = 160 * 1024;
constexpr int kSeedKD = 12;      // compressed dimensions of the support-seed problem (amx_seed.hpp)
constexpr int kSeedLd = 14;      // LDS row stride of S (odd: per-lane column gathers spread over the banks)
constexpr int kSeed2KD = 8;      // components the LASSO seed solver works with (the first 8 of the 12 stored: the pivoted basis is nested)
constexpr int kSeed3ListRow = 36;      // bytes per lane of the stage-3 candidate lists in LDS (k_nnls_seed<3>)
// rows of a block of the A'y table (k_noddi_gemm, amx_seed.hpp): atoms 0 .. n_atoms - 1, then from aux0 = n_atoms: U'y (12), U2'y (12),
// sum_b0 y, ||y||^2, sum_b0 y^2, t_min = min_dwi y_i / iso_i; padded to whole 16-row MFMA tiles
constexpr int kAuxU = 0, kAuxU2 = 12, kAuxB0 = 24, kAuxYY = 25, kAuxYB = 26, kAuxTmin = 27, kAuxN = 28;
constexpr int gemm_rows(int n_atoms) { return ((n_atoms + kAuxN + 15) / 16) * 16; }
constexpr int kScreenLd = 192;   // atoms per row of the float32 screening table [KD][kScreenLd]
constexpr size_t kScreenBytes = (size_t)kSeedKD * kScreenLd * sizeof(float);   // ... which a stage kernel that screens holds in LDS (amx_solver.hpp, amx_gram_solver.hpp)

// doubles of per-wavefront LDS the solver needs besides the residual scratch:
// QR solver: R and the ridge rows, (MAXP+1)^2 each; Gram solver: two packed triangles
// (without the ridge the QR solver has no augmented rows: R only)
constexpr int solver_lds_words(bool gram, int maxp, bool ridge = true)
{
    return gram ? (maxp + 1) * (maxp + 2) : (ridge ? 2 : 1) * (maxp + 1) * (maxp + 1);
}

// dynamic LDS of a wavefront-per-voxel kernel (amx_kernels.hpp: AMX_KERNEL_PROLOGUE): the tile in elements of `elem` bytes (none for the
// global-tile builds), then per wavefront the signal rows, the solver's block and four mask words; 16 spare bytes (the ticket)
inline size_t fit_lds_bytes(size_t elem, int nS, int ldA, int NR, int NQ, int NW, int MAXP, bool gram = false, bool ridge = true, bool global_tile = false)
{
    const size_t words_pad = global_tile ? 0 : (((size_t)nS * ldA + kWave * NQ + 3) & ~(size_t)3);
    size_t b = (words_pad * elem + 15) & ~(size_t)15;
    b += (size_t)NW * NR * kWave * sizeof(double);
    b += (size_t)NW * solver_lds_words(gram, MAXP, ridge) * sizeof(double);
    b += (size_t)NW * 4 * sizeof(unsigned long long);
    b += 16;
    return b;
}
template <typename AT>
inline size_t fit_lds_bytes(int nS, int ldA, int NR, int NQ, int NW, int MAXP, bool gram = false, bool ridge = true, bool global_tile = false)
{
    return fit_lds_bytes(sizeof(AT), nS, ldA, NR, NQ, NW, MAXP, gram, ridge, global_tile);
}

// LDS of k_noddi_gemm for a dictionary shape and K-steps: float32 tiles of atoms only, fp64 tiles for the rest, iso table, column scales
inline size_t gemm_lds(int n_cols, int rows, int ks)
{
    const int mtf = n_cols / 16, mt = rows / 16;
    return (size_t)mtf * ks * 64 * sizeof(float) + ((size_t)(mt - mtf) * ks * 64 + 4 * ks + rows + 2) * sizeof(double);   // (+ the workgroup's next chunk)
}
// Protocols of more than 160 volumes take several launches, each over a window of <= 160 samples of every voxel (GemmArgs::k0, k1):
// 288 volumes = 2 windows of 144, 512 = 4 of 128.
inline int gemm_passes(int nS) { return (nS + 159) / 160; }
inline int gemm_window(int nS) { const int np = gemm_passes(nS); return ((nS + np - 1) / np + 3) & ~3; }   // samples per window, a multiple of 4

// ------------------------------------------------------------------ FreeWater, SANDI, CylinderZeppelinBall (routed by amx_small_route.hpp)
// dynamic LDS of a lane-per-voxel kernel (amx_lane_qp.hpp: AMX_SMALL_LDS): the tile in elements of `elem` bytes, then H [N][N]
inline size_t lane_lds_bytes(size_t elem, int nS, int ldA, int N) { return (((size_t)nS * ldA * elem + 15) & ~(size_t)15) + (size_t)N * N * sizeof(double); }
// FreeWater's projection kernels (amx_fw_lane.hip)
constexpr int kTileRows = 16;          // signal values per voxel and transposition pass
constexpr int kTileLd = 65;            // odd leading dimension (doubles) of the transposition tile [row][voxel]
constexpr int kProjKS = 24;            // K-steps of dictionary registers of the matrix-core projection: nS <= 4 kProjKS = 96
// k_fw_project: Ad f64 [nS][NP] | Hi f64 [N][NP] | per wavefront: Tt [kTileRows][kTileLd], Vb int[64]
inline size_t fw_project_lds_bytes(int nS, int N, int nw)
{
    const int NP = (N + 1) & ~1;
    return ((size_t)(nS + N) * NP + (size_t)nw * (kTileRows * kTileLd + 32)) * sizeof(double);
}
// k_enet_big (amx_bpp.hpp: Work): the workgroup's vectors in LDS, one block of vec_bytes(m, n) bytes
namespace bpp {
constexpr int kThreads = 256;
constexpr size_t vec_bytes(int m, int n)
{
    const size_t mp = (size_t)((m + 1) & ~1), npd = (size_t)((n + 1) & ~1), n4 = (size_t)((n + 3) & ~3);
    return ((2 * mp + 9 * npd + kThreads + 2) * sizeof(double) + (5 * n4 + 16) * sizeof(int) + 15) & ~(size_t)15;
}
}  // namespace bpp

}  // namespace amx

constexpr int kChunk = 256;        // voxels of one orientation per workgroup
// Lane-per-voxel solvers: start the active set from ALL atoms and drop the non-positive ones in blocks (unique optimum
// with lambda2 > 0, so the path is free; dense optima are reached in 3-4 factorisations).  Flag bit 31 asks for the Lawson-Hanson start from
// the empty set instead (a retired A/B switch set it; no caller does).  Needs a ridge that keeps the full system well conditioned.
constexpr bool amx_warm_start(double lam2, unsigned flags) { return lam2 >= 1e-5 && !(flags & 0x80000000u); }
