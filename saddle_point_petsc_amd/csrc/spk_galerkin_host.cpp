// spk_galerkin_host.cpp -- the grid-stencil Galerkin product (SPK_AMG_GALERKIN_STENCIL) in plain loops over the functions
// of spk_galerkin_core.hpp: the host route's step (spk_amg_host.cpp: HostRoute::stencil) and the oracle of the kernels
// (spk_k_amg_setup.hip: amgs_galerkin_stencil...).  Host-pure like spk_host.cpp, whose header declares these: the standard
// library, include/spk.h and the core header only; exercised without a GPU by tests/host/galerkin_stencil_check.cpp.
#include "spk_host.hpp"
#include "spk_galerkin_core.hpp"

namespace spk {

namespace gs = galerkin;

void galerkin_stencil_check_host(const int32_t fd[3], int bs, const int32_t *arp, const int32_t *aci)
{
    const int64_t n = (int64_t)fd[0] * fd[1] * fd[2] * bs;
    for (int64_t r = 0; r < n; ++r) {
        const int32_t c = gs::gs_check_row(fd, bs, arp, aci, r);
        if (c >= 0)
            fail(SPK_ERR_UNSUPPORTED, "amg: the entry in row %lld, column %d of the operator couples nodes that are not neighbours "
                 "on the %d x %d x %d grid; the stencil products take couplings between neighbouring nodes only -- use "
                 "-spk_mg_galerkin products", (long long)r, (int)c, (int)fd[0], (int)fd[1], (int)fd[2]);
    }
}

template <int BS>
static void galerkin_stencil_bs(const gs::GsGrid &g, const int32_t cd[3], const int32_t *arp, const int32_t *aci, const double *av,
                                int32_t *rp, int32_t *ci, double *v)
{
    const int64_t items = gs::gs_items(cd, BS);
    parallel_for(items, [&](int64_t b, int64_t e, int) {
        gs::GsItem it;
        for (int64_t t = b; t < e; ++t)
            if (gs::gs_item(cd, BS, t, &it)) gs::gs_gather<BS>(g, arp, aci, av, it, rp, ci, v);
    });
    parallel_for(items, [&](int64_t b, int64_t e, int) {   // (no two items share a pair: any split is race-free)
        gs::GsItem it;
        for (int64_t t = b; t < e; ++t)
            if (gs::gs_item(cd, BS, t, &it)) gs::gs_symmetrise<BS>(cd, it, v);
    });
}

void galerkin_stencil_host(const int32_t fd[3], const int32_t cd[3], int bs, const int32_t *arp, const int32_t *aci, const double *av,
                           int32_t *rp, int32_t *ci, double *v)
{
    const gs::GsGrid g = gs::gs_grid(fd, cd);
    if (bs == 1) galerkin_stencil_bs<1>(g, cd, arp, aci, av, rp, ci, v);
    else if (bs == 2) galerkin_stencil_bs<2>(g, cd, arp, aci, av, rp, ci, v);
    else if (bs == 3) galerkin_stencil_bs<3>(g, cd, arp, aci, av, rp, ci, v);
    else fail(SPK_ERR_ARG, "amg: the stencil products take node sizes 1, 2 and 3, not %d", bs);
}

int galerkin_stencil_children(const int32_t fd[3], const int32_t cd[3], int32_t node, int32_t *nodes, double *w)
{
    const gs::GsGrid g = gs::gs_grid(fd, cd);
    const int32_t i = node % cd[0], j = (node / cd[0]) % cd[1], k = node / cd[0] / cd[1];
    int32_t lo[3], hi[3], n = 0;
    gs::gs_children(g.d[0], i, &lo[0], &hi[0]);
    gs::gs_children(g.d[1], j, &lo[1], &hi[1]);
    gs::gs_children(g.d[2], k, &lo[2], &hi[2]);
    for (int32_t z = lo[2]; z <= hi[2]; ++z)
        for (int32_t y = lo[1]; y <= hi[1]; ++y)
            for (int32_t x = lo[0]; x <= hi[0]; ++x, ++n) {
                if (nodes) nodes[n] = (z * fd[1] + y) * fd[0] + x;
                if (w) w[n] = gs::gs_weight(g.d[2], z, k) * gs::gs_weight(g.d[1], y, j) * gs::gs_weight(g.d[0], x, i);
            }
    return n;
}

}  // namespace spk
