// amx_unring_route.hpp -- what the Gibbs-unringing kernels (amx_unring.hip) ask for a slice of n_a x n_b pixels, as plain
// arithmetic (no HIP in here): amx_prep_unring_device launches by it and amx_unring_route hands it out, so a test without a GPU can walk
// every pair of extents.
#pragma once
#include <stddef.h>

namespace amx {

constexpr int kUnringMin = 8, kUnringMax = 256;            // in-plane extents the kernels take
constexpr int kUnringShifts = 41;                          // s = 0, then j / 40 and -j / 40 for j = 1 .. 20
constexpr int kUnringTile = 16;                            // rows of a tile of the 16x16x4 fp64 MFMA ...
constexpr int kUnringLines = 16;                           // ... its columns: the image lines a workgroup takes
constexpr int kUnringK = 4;                                // ... and its depth
constexpr int kUnringLd = kUnringLines + 1;                // words between the rows of a staged tile of lines (odd: no bank conflict either way)
constexpr int kUnringThreads = 256;                        // a workgroup: four wavefronts
constexpr size_t kUnringLdsMax = 160 * 1024;               // bytes of LDS a workgroup may ask for on gfx950
constexpr size_t kUnringScratchCap = (size_t)128 << 20;    // bytes of ctx workspace a call may hold, whatever the number of slices
constexpr int kUnringPlanes = 5;                           // float64 planes of a slice in flight: the slice, two complex pairs

struct UnringRoute {
    int ok;                 // 0: refused (an extent outside [kUnringMin, kUnringMax])
    int pad_a, pad_b;       // the extents rounded up to the tile: rows of zeros, never a cyclic index
    int tiles_a, tiles_b;   // row tiles of a line along a / b
    int groups_a, groups_b; // workgroups of a slice for lines along a (there are n_b of them) / along b (n_a)
    size_t lds_dft;         // bytes per workgroup of k_unring_dft: a tile of complex lines
    size_t lds_shift;       // bytes per workgroup of k_unring_shift: the lines, their shifted copy, one row of the shift table
    size_t table_bytes;     // cosine and sine tables of both axes, both shift tables
    size_t slice_bytes;     // float64 scratch of one slice (kUnringPlanes planes) and its flag
    long long chunk;        // slices per chunk: table_bytes + chunk * slice_bytes <= kUnringScratchCap
};

inline UnringRoute unring_route(int n_a, int n_b)
{
    UnringRoute rt = {};
    if (n_a < kUnringMin || n_a > kUnringMax || n_b < kUnringMin || n_b > kUnringMax) return rt;
    rt.ok = 1;
    rt.tiles_a = (n_a + kUnringTile - 1) / kUnringTile; rt.tiles_b = (n_b + kUnringTile - 1) / kUnringTile;
    rt.pad_a = rt.tiles_a * kUnringTile; rt.pad_b = rt.tiles_b * kUnringTile;
    rt.groups_a = (n_b + kUnringLines - 1) / kUnringLines; rt.groups_b = (n_a + kUnringLines - 1) / kUnringLines;
    const int pad = rt.pad_a > rt.pad_b ? rt.pad_a : rt.pad_b, nmax = n_a > n_b ? n_a : n_b;
    rt.lds_dft = (size_t)2 * pad * kUnringLd * 8;
    rt.lds_shift = (size_t)2 * pad * kUnringLd * 8 + (size_t)nmax * 8;
    rt.table_bytes = 512 + ((size_t)2 * n_a * n_a + (size_t)2 * n_b * n_b + (size_t)kUnringShifts * (n_a + n_b)) * 8;
    rt.slice_bytes = (size_t)kUnringPlanes * n_a * n_b * 8 + 8;
    // (the grow-only workspace asks for bytes + bytes / 8 + 256: that is what stays under the cap)
    rt.chunk = (long long)(((kUnringScratchCap - 256) / 9 * 8 - rt.table_bytes) / rt.slice_bytes);
    if (rt.lds_dft > kUnringLdsMax || rt.lds_shift > kUnringLdsMax || rt.chunk < 1) rt.ok = 0;
    return rt;
}

}  // namespace amx
