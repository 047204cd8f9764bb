// amx_prep_route.hpp -- which tile kernel a gather plan launches and what LDS it asks for, as plain arithmetic (no HIP in here):
// prep_gather_dev launches by it and amx_prep_route hands it out, so a test without a GPU can walk every volume count.
#pragma once
#include <stddef.h>

namespace amx {

constexpr int kDirectLd = 65;               // words per volume row of the direct-load tile T[volume][voxel]
constexpr int kPrepWaves = 2;               // wavefronts per workgroup of k_prep_gather, one 64-voxel tile each
constexpr int kPrepLongChunk = 64;          // k_prep_long, groups not in place: output volumes per pass of the O[voxel][chunk] tile
constexpr int kPrepLongChunkLd = kPrepLongChunk + 1;
constexpr int kPrepMaxVolumes = 512;        // the fits' own limit (amx_lut_upload_*): the long route ends where they do
constexpr size_t kPrepLdsMax = 160 * 1024;  // bytes of LDS a workgroup may ask for on gfx950

enum { PREP_ROUTE_REFUSED = 0, PREP_ROUTE_TILE = 1, PREP_ROUTE_LONG = 2 };

struct PrepRoute {
    int route;          // PREP_ROUTE_*
    int waves;          // wavefronts (= tiles) per workgroup
    size_t per_wave;    // words of one wavefront's tile(s)
    size_t lds;         // bytes per workgroup, the plan's index lists included
};

// identity: every output volume is its input volume; direct: identity on a layout that is not interleaved (tile T[volume][voxel]);
// inplace: a group's output may replace input volume j of the tile (amx_prep::inplace).
//  TILE: k_prep_gather, two wavefronts per workgroup, each with all nS samples of its 64 voxels (and, groups not in place, all
//        n_out outputs beside them) -- chosen whenever that fits, exactly as before the long route existed;
//  LONG: k_prep_long, ONE wavefront per workgroup with the same tile; groups not in place get kPrepLongChunk output volumes at a
//        time in a small second tile instead of all n_out;
//  REFUSED: more than kPrepMaxVolumes volumes (or lists so long that even the one tile does not fit).
inline PrepRoute prep_route(int nS, int n_out, int n_b0, int n_gidx, bool identity, bool direct, bool inplace)
{
    const size_t ldt = (size_t)(nS | 1);
    const size_t tile = (identity && direct) ? (size_t)nS * kDirectLd : (size_t)64 * ldt;
    const size_t lists = (size_t)n_b0 + (size_t)n_out + 1 + (size_t)n_gidx;
    PrepRoute r;
    r.route = PREP_ROUTE_TILE; r.waves = kPrepWaves;
    r.per_wave = (identity || inplace) ? tile : 2 * tile;
    r.lds = ((size_t)kPrepWaves * r.per_wave + lists) * sizeof(float);
    if (r.lds <= kPrepLdsMax) return r;
    r.route = PREP_ROUTE_LONG; r.waves = 1;
    r.per_wave = (identity || inplace) ? tile : tile + (size_t)64 * kPrepLongChunkLd;
    r.lds = (r.per_wave + lists) * sizeof(float);
    if (nS > kPrepMaxVolumes || r.lds > kPrepLdsMax) r.route = PREP_ROUTE_REFUSED;
    return r;
}

}  // namespace amx
