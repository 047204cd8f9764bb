// amx_fw.hip -- FreeWater (models.pyx:1231-1276): the solver the fit's route names (amx_small_route.hpp).  Here the wavefront-per-voxel kernel
// (amx_kernels.hpp); the lane-per-voxel kernels of the small dictionaries, the fast path, are in amx_fw_lane.hip
#include "amx_launch.hpp"
using namespace amx;

template <int NR>
static int go(amx_ctx *ctx, FwArgs &a, const Plan &pl, hipStream_t s, const SmallRoute &rt)
{
    constexpr int NQ = 1, MP = 16, MB = 64;      // (small_route sizes the LDS with the same three)
    constexpr int NW = 8;
    return launch_pair<NW>(ctx, a, pl, s, k_freewater<NR, NQ, MP, NW, false>, k_freewater<NR, NQ, MB, 1, true>, route_lds(rt.waves, rt.lds), rt.lds_list, 0, 2, rt.launch[0]);
}

int amx_launch_fw(amx_ctx *ctx, FwArgs &a, const Plan &pl, hipStream_t s, const SmallRoute &rt)
{
    if (rt.family != SF_WAVE) return amx_launch_fw_small(ctx, a, pl, s, rt);
    return rt.NR == 2 ? go<2>(ctx, a, pl, s, rt) : (rt.NR == 4 ? go<4>(ctx, a, pl, s, rt) : go<8>(ctx, a, pl, s, rt));
}
