// amx_noddi_s1.hip -- NODDI solver stage 1 (models.pyx:911).  Which build runs, with how many wavefronts and how much LDS, and why:
// amx_noddi_route.hpp (noddi_nnls_kernel)
#include "amx_launch.hpp"
using namespace amx;

template <int NR>
static int go(amx_ctx *ctx, NoddiArgs &a, const Plan &pl, hipStream_t s, const NoddiKernel &k)
{
    constexpr int NQ = 3, MP = 8, MB = 32, NW = 16;
    switch (k.build) {
    case NB_SMALL: return launch_pair<4>(ctx, a, pl, s, k_noddi<1, NR, NQ, 12, 4, false, float>, k_noddi<1, NR, NQ, MB, 1, true>, route_lds(k), k.lds_list, 0, 2, k.note);
    case NB_F32_8: if constexpr (NR == 4) return launch_pair<8>(ctx, a, pl, s, k_noddi<1, NR, NQ, 12, 8, false, float>, k_noddi<1, NR, NQ, MB, 1, true>, route_lds(k), k.lds_list, 0, 2, k.note); break;
    case NB_F64_12: return launch_pair<12>(ctx, a, pl, s, k_noddi<1, NR, NQ, 12, 12, false, double>, k_noddi<1, NR, NQ, MB, 1, true>, route_lds(k), k.lds_list, 0, 2, k.note);
    case NB_F64_NW: return launch_pair<NW>(ctx, a, pl, s, k_noddi<1, NR, NQ, MP, NW, false, double>, k_noddi<1, NR, NQ, MB, 1, true>, route_lds(k), k.lds_list, 0, 2, k.note);
    case NB_F32_NW: return launch_pair<NW>(ctx, a, pl, s, k_noddi<1, NR, NQ, MP, NW, false>, k_noddi<1, NR, NQ, MB, 1, true>, route_lds(k), k.lds_list, 0, 2, k.note);
    }
    return amx_bad(ctx, "k_noddi<1>: no such build");
}

int amx_launch_noddi_s1(amx_ctx *ctx, NoddiArgs &a, const Plan &pl, hipStream_t s, const NoddiKernel &k)
{
    if (k.build == NB_GLOBAL)
        return launch_pair<4>(ctx, a, pl, s, k_noddi<1, 8, 4, 12, 4, false, float, true>, k_noddi<1, 8, 4, 32, 1, true, float, true>, route_lds(k), k.lds_list, 0, 2, k.note);
    return k.NR == 2 ? go<2>(ctx, a, pl, s, k) : go<4>(ctx, a, pl, s, k);
}
