// amx_mppca_route.hpp -- the shape of one Marchenko-Pastur patch problem and what k_mppca asks of a workgroup for it, as plain arithmetic
// (no HIP in here): amx_prep_noise_mppca_device launches by it and amx_mppca_route hands it out, so a test without a GPU can walk every
// (volumes, patch edge, masked columns) combination.
#pragma once
#include <stddef.h>

namespace amx {

constexpr int kMppcaMaxVolumes = 512;        // the fits' and the gather's own limit
constexpr int kMppcaMaxSide = 125;           // 5^3: the largest Gram matrix, and the row length of d_eig
constexpr int kMppcaChunk = 32;              // samples of every Gram row staged at a time (8 K-steps of the 16x16x4 fp64 MFMA)
constexpr int kMppcaThreads = 256;           // a workgroup: four wavefronts
constexpr size_t kMppcaLdsMax = 160 * 1024;  // bytes of LDS a workgroup may ask for on gfx950

enum { MPPCA_SIDE_VOLUMES = 0, MPPCA_SIDE_PATCH = 1 };   // G = X X^T over the volumes (m <= n) | X^T X over the patch's voxels (m > n)

struct MppcaRoute {
    int ok;             // 0: refused
    int r, q;           // min / max of (volumes m, masked columns n)
    int side;           // MPPCA_SIDE_*
    int gram;           // order of G (= r)
    int chunk;          // samples per staged chunk; ceil(q / chunk) chunks
    int waves;          // wavefronts that share one patch
    int patches;        // patches per workgroup
    int eligible;       // 2 n >= w^3
    size_t per_patch;   // LDS bytes of one patch's team (sized for the launch: r_max = min(m, w^3))
    size_t lds;         // LDS bytes per workgroup
};

// LDS of one patch, sized for r_max = min(nS, w^3), rp = r_max rounded up to the MFMA tile:
//   G [r_max][r_max | 1] f64, seven vectors [rp] f64 (d, e, v, w, eigenvalues, two partial sums), the columns' image offsets [w^3] i64,
//   the staging tile [rp][chunk + 1] f32, 16 words of state
inline size_t mppca_patch_bytes(int nS, int w)
{
    const int w3 = w * w * w, rmax = nS < w3 ? nS : w3, rp = (rmax + 15) / 16 * 16;
    return (size_t)rmax * (size_t)(rmax | 1) * 8 + (size_t)7 * rp * 8 + (size_t)w3 * 8 + (size_t)rp * (kMppcaChunk + 1) * 4 + 64;
}

// d: the three spatial extents (any order); n: masked voxels in the cube (the columns)
inline MppcaRoute mppca_route(int nS, int w, int n, long long d0, long long d1, long long d2)
{
    MppcaRoute rt = {};
    if ((w != 3 && w != 5) || nS < 1 || nS > kMppcaMaxVolumes || d0 < w || d1 < w || d2 < w || n < 0 || n > w * w * w) return rt;
    rt.ok = 1;
    rt.r = nS < n ? nS : n; rt.q = nS < n ? n : nS;
    rt.side = nS <= n ? MPPCA_SIDE_VOLUMES : MPPCA_SIDE_PATCH;
    rt.gram = rt.r;
    rt.chunk = kMppcaChunk;
    rt.waves = w == 5 ? 4 : 1;                  // w = 3: G is under 6 KB, a wavefront per patch and four patches per workgroup
    rt.patches = kMppcaThreads / 64 / rt.waves;
    rt.eligible = 2 * n >= w * w * w;
    rt.per_patch = mppca_patch_bytes(nS, w);
    rt.lds = rt.per_patch * rt.patches;
    if (rt.lds > kMppcaLdsMax) rt.ok = 0;
    return rt;
}

// k_mppca_denoise: k_mppca's team shapes and LDS, and one more [rp] vector (the reflectors' tau2).  The eigenvectors live in what the
// tridiagonalisation leaves dead of G (its lower triangle with the diagonal): (r - 1) / 2 + 1 vectors of r words, and the smaller of the
// signal and the noise set never has more than r / 2 -- so no route has a cap.
struct MppcaDenoiseRoute {
    int ok;             // 0: refused (what mppca_route refuses)
    int r, q, side;     // as MppcaRoute
    int waves, patches; // as MppcaRoute
    int eligible;       // 2 n >= w^3
    int capacity;       // eigenvectors of length r the dead triangle of G holds
    int cap;            // the most min(n_signal, r - n_signal) may be; 0: no cap (a voxel above a cap would be passed through, status 2)
    size_t per_patch;   // LDS bytes of one patch's team
    size_t lds;         // LDS bytes per workgroup
};

inline MppcaDenoiseRoute mppca_denoise_route(int nS, int w, int n, long long d0, long long d1, long long d2)
{
    MppcaDenoiseRoute rt = {};
    const MppcaRoute base = mppca_route(nS, w, n, d0, d1, d2);
    if (!base.ok) return rt;
    const int w3 = w * w * w, rmax = nS < w3 ? nS : w3, rp = (rmax + 15) / 16 * 16;
    rt.ok = 1;
    rt.r = base.r; rt.q = base.q; rt.side = base.side; rt.waves = base.waves; rt.patches = base.patches; rt.eligible = base.eligible;
    rt.capacity = rt.r > 0 ? (rt.r - 1) / 2 + 1 : 0;
    rt.cap = 0;
    rt.per_patch = base.per_patch + (size_t)rp * 8;
    rt.lds = rt.per_patch * rt.patches;
    if (rt.lds > kMppcaLdsMax) rt.ok = 0;
    return rt;
}

}  // namespace amx
