// amx_sandi.hip -- SANDI (models.pyx:1567-1619): the solver the fit's route names (amx_small_route.hpp).  Here the wavefront-per-voxel kernel
// (amx_kernels.hpp); the lane-per-voxel kernels of the small dictionaries, the fast path, are in amx_sandi_lane.hip
#include "amx_launch.hpp"
using namespace amx;

template <int NR>
static int go(amx_ctx *ctx, SandiArgs &a, const Plan &pl, hipStream_t s, const SmallRoute &rt)
{
    constexpr int NQ = 1, MP = 16, MB = 64;      // (small_route sizes the LDS with the same three)
    constexpr int NW = 8;
    return launch_pair<NW>(ctx, a, pl, s, k_sandi<NR, NQ, MP, NW, false>, k_sandi<NR, NQ, MB, 1, true>, route_lds(rt.waves, rt.lds), rt.lds_list, 0, 2, rt.launch[0]);
}

int amx_launch_sandi(amx_ctx *ctx, SandiArgs &a, const Plan &pl, hipStream_t s, const SmallRoute &rt)
{
    if (rt.family != SF_WAVE) return amx_launch_sandi_small(ctx, a, pl, s, rt);
    return rt.NR == 1 ? go<1>(ctx, a, pl, s, rt) : go<2>(ctx, a, pl, s, rt);
}
