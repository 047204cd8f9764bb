// amx_noddi_s2.hip -- NODDI solver stage 2, the LASSO (models.pyx:914-926): the Gram-space variant (amx_gram_solver.hpp), the QR (A-space)
// variant for any lambda2 > 0, or straight to k_noddi_lasso_big.  Which one, with how many wavefronts and how much LDS, and why:
// amx_noddi_route.hpp (noddi_lasso_kernel)
#include "amx_launch.hpp"
using namespace amx;

template <int NR>
static int go(amx_ctx *ctx, NoddiArgs &a, const Plan &pl, hipStream_t s, const NoddiKernel &k)
{
    constexpr int NQ = 3, MP = 20, MB = 64;
    switch (k.build) {
    case NB_QR: return launch_pair<8>(ctx, a, pl, s, k_noddi<2, NR, NQ, MP, 8, false>, k_noddi<2, NR, NQ, MB, 1, true>, route_lds(k), k.lds_list, 1, 4, k.note);
    case NB_GRAM_LEFT: return launch_pair<8>(ctx, a, pl, s, k_noddi<4, NR, NQ, 32, 8, false>, k_noddi<4, NR, NQ, MB, 1, true>, route_lds(k), k.lds_list, 1, 4, k.note, true);
    case NB_GRAM: return launch_pair<16>(ctx, a, pl, s, k_noddi<4, NR, NQ, MP, 16, false>, k_noddi<4, NR, NQ, MB, 1, true>, route_lds(k), k.lds_list, 1, 4, k.note, true);
    }
    return amx_bad(ctx, "k_noddi<4|2>: no such build");
}

int amx_launch_noddi_s2(amx_ctx *ctx, NoddiArgs &a, const Plan &pl, hipStream_t s, const NoddiKernel &k)
{
    int rc;
    if (k.build == NB_BIG_ALL) return amx_launch_noddi_big(ctx, a, pl, s, nullptr, nullptr, (int)pl.n);
    if (k.build == NB_GLOBAL && k.gram)
        rc = launch_pair<4>(ctx, a, pl, s, k_noddi<4, 8, 4, 32, 4, false, float, true>, k_noddi<4, 8, 4, 64, 1, true, float, true>, route_lds(k), k.lds_list, 1, 4, k.note, true);
    else if (k.build == NB_GLOBAL)
        rc = launch_pair<4>(ctx, a, pl, s, k_noddi<2, 8, 4, 20, 4, false, float, true>, k_noddi<2, 8, 4, 32, 1, true, float, true>, route_lds(k), k.lds_list, 1, 4, k.note);
    else rc = k.NR == 2 ? go<2>(ctx, a, pl, s, k) : go<4>(ctx, a, pl, s, k);
    if (rc || !k.gram) return rc;
    // supports of more than 64 atoms (a weak lambda1: the optimum is dense): the slow exact solver, from the re-run kernel's own overflow list
    return amx_launch_noddi_big(ctx, a, pl, s, pl.ovf_list + (size_t)6 * pl.n, pl.ovf_count + 10, 0);
}
