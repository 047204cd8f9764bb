// amx_lut_route.hpp -- which of the three LUT resampling GEMM kernels a shape launches, with which compile-time reduction length and
// how much LDS, as plain arithmetic (no HIP in here): lut_gemm launches by it and amx_lut_route hands it out, so a test without a GPU
// can walk every (K, N) and a GPU test can say which kernel it is about to hold to its reference.
#pragma once
#include <stddef.h>

namespace amx {

constexpr int kLutKhMax = 64;                  // largest compile-time half-length: K <= 4 * 64 reduction indices in registers / LDS
constexpr size_t kLutLdsTileMax = 160 * 1024;  // k_lut_resample_tile: operator zone + four row tiles, one workgroup per CU
constexpr size_t kLutLdsMax = 80 * 1024;       // k_lut_resample: the padded operator alone, two workgroups per CU

enum { LUT_ROUTE_REFUSED = 0, LUT_ROUTE_TILE = 1, LUT_ROUTE_LDS = 2, LUT_ROUTE_GENERIC = 3 };

struct LutRoute {
    int route;          // LUT_ROUTE_*
    int kh2;            // template argument KH2 of the tile / lds kernels: 23, 46 or 64 pairs per half-wavefront (1 / 2 shells of lmax 12, <= 256)
    size_t lds;         // dynamic LDS bytes per workgroup (0: generic, refused)
};

// n_sh = K reduction indices (SH coefficients x shells), n_out = N DWI volumes; fused: the left operand is formed in registers from
// (zonal x basis) factors (amx_lut_rotate_resample) instead of being read from memory.
//  TILE:    k_lut_resample_tile -- plain input, K even, at most 4 floats of padding up to 4 * kh2 (a row is read that far beyond its end),
//           operator zone (whole KB + 2 KB of zeros) and four 32-row tiles (whole KB each) within 160 KB;
//  LDS:     k_lut_resample -- K <= 256 and the operator, padded to [N up to 32][4 * kh2 + 2] floats, within 80 KB; the only fused kernel;
//  GENERIC: k_lut_resample_generic -- everything else that is plain input, operands from L2;
//  REFUSED: a fused shape beyond the LDS route.
inline LutRoute lut_route(int n_sh, int n_out, bool fused)
{
    LutRoute r;
    const long long kh2 = ((long long)n_sh + 3) / 4;               // (sizes of any int: no sum in here overflows)
    r.kh2 = kh2 <= 23 ? 23 : (kh2 <= 46 ? 46 : kLutKhMax);
    const size_t lds = (((size_t)n_out + 31) & ~(size_t)31) * (4 * r.kh2 + 2) * sizeof(float);
    const size_t yzone = ((((size_t)n_out * n_sh * 4) + 1023) & ~(size_t)1023) + 2048;
    const size_t lds_tile = yzone + 4 * ((((size_t)32 * n_sh * 4) + 1023) & ~(size_t)1023);
    if (!fused && (n_sh & 1) == 0 && n_sh <= 4 * kLutKhMax && 4 * r.kh2 - n_sh <= 4 && lds_tile <= kLutLdsTileMax) {
        r.route = LUT_ROUTE_TILE; r.lds = lds_tile;
    } else if (n_sh > 4 * kLutKhMax || lds > kLutLdsMax) {
        r.route = fused ? LUT_ROUTE_REFUSED : LUT_ROUTE_GENERIC; r.lds = 0;
    } else {
        r.route = LUT_ROUTE_LDS; r.lds = lds;
    }
    return r;
}

}  // namespace amx
