// constraints_core_check.cpp -- self-checking program over csrc/spk_constraints_core.hpp, the closed forms the kernels of
// spk_k_constraints.hip execute.  For every grid with sides 3..10 (2-D) and 3..6 (3-D) and every slab of whole node lines
// or planes -- slabs of boundary lines only and empty slabs included -- it runs the three kernels' bodies on the CPU,
// "thread" by "thread", into arrays allocated at exactly their sizes, and compares them byte for byte with what the host
// chain produces: the generator (spk_assembly.cpp), then localise_and_sort, wide_rows, window_pointers and
// transpose_rows (spk_host.cpp).  The window pointers are compared at the width window_width chooses and at narrow
// widths, so that rows are cut inside a node, inside a line and at a plane.  A failed check prints the case and the
// program exits with status 1.  Built by tests/test_constraints_core_cpu.py, once more with the sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/spk_assembly.h"
#include "spk_constraints_core.hpp"
#include "spk_host.hpp"

using namespace spk;
namespace cs = spk::constraints;

static int g_failed = 0, g_cases = 0;
static char g_case[128];
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::printf("FAILED %s: %s (line %d)\n", g_case, #cond, __LINE__);            \
            ++g_failed;                                                                    \
        }                                                                                  \
    } while (0)

template <class T>
static bool same(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

static void one_slab(int mx, int my, int mz, int u0, int u1)
{
    ++g_cases;
    std::snprintf(g_case, sizeof g_case, "%d x %d x %d units [%d,%d)", mx, my, mz, u0, u1);
    const int64_t unit_rows = mz ? 3 * (int64_t)mx * my : 2 * (int64_t)mx;
    const int64_t rb = u0 * unit_rows, re = u1 * unit_rows;
    const int32_t m = mz ? 6 : 4, nl = (int32_t)(re - rb);
    // ---- the host chain
    const int64_t nnz = mz ? SpkConstraintsSlabNnz3D(mx, my, mz, rb, re) : SpkConstraintsSlabNnz(mx, my, rb, re);
    CHECK(nnz >= 0);
    if (nnz < 0) return;
    std::vector<int32_t> rowptr((size_t)m + 1), gcol((size_t)nnz);
    std::vector<double> gval((size_t)nnz);
    int32_t none_i = 0;
    double none_d = 0.0;   // (the generator refuses null arrays, an empty slab's included)
    CHECK((mz ? SpkAssembleOperator_Constraints3D(mx, my, mz, rb, re, rowptr.data(), nnz ? gcol.data() : &none_i, nnz ? gval.data() : &none_d)
              : SpkAssembleOperator_Constraints(mx, my, rb, re, rowptr.data(), nnz ? gcol.data() : &none_i, nnz ? gval.data() : &none_d)) == 0);
    std::vector<int32_t> hcol((size_t)nnz), htrp((size_t)nl + 1, 0), htci((size_t)nnz);
    std::vector<double> hval((size_t)nnz), htv((size_t)nnz);
    localise_and_sort(m, rowptr.data(), gcol.data(), gval.data(), rb, re, hcol.data(), hval.data());
    const std::vector<int32_t> wide = wide_rows(m, rowptr.data(), 8192);
    CHECK((int32_t)wide.size() == m);
    for (int32_t r = 0; r < m && r < (int32_t)wide.size(); ++r) CHECK(wide[(size_t)r] == r);
    transpose_rows(m, nl, rowptr.data(), hcol.data(), hval.data(), htrp.data(), htci.data(), htv.data());

    // ---- the core, as the kernels call it
    const cs::Slab g{mx, my, mz, u0, u1};
    CHECK(cs::rows(g) == m && cs::local_cols(g) == nl && cs::nnz(g) == nnz);
    const int64_t nint = cs::row_count(g);
    for (int32_t r = 0; r <= m; ++r) CHECK(rowptr[(size_t)r] == r * nint);   // the entry count of every row
    std::vector<int32_t> dcol((size_t)nnz), dtrp((size_t)nl + 1), dtci((size_t)nnz);
    std::vector<double> dval((size_t)nnz), dtv((size_t)nnz);
    const double w = cs::weight(g);
    for (int64_t q = 0; q < nint; ++q) {   // constraints_b_kernel
        const cs::Node nd = cs::interior_node(g, q);
        for (int r = 0; r < m; ++r) {
            const int64_t p = cs::b_position(g, r, q);
            CHECK(p >= 0 && p < nnz);
            if (p < 0 || p >= nnz) return;
            dcol[(size_t)p] = cs::b_column(g, r, nd);
            dval[(size_t)p] = cs::value(g, w, r, nd);
        }
    }
    for (int64_t lr = 0; lr <= nl; ++lr) {   // constraints_bt_kernel
        const int64_t p = cs::bt_rowptr(g, lr);
        dtrp[(size_t)lr] = (int32_t)p;
        if (lr == nl) break;
        const int d = cs::dof(g);
        const int64_t N = lr / d;
        const int c = (int)(lr - N * d);
        bool in;
        const cs::Node nd = cs::local_node(g, N, in);
        if (!in) continue;
        CHECK(p >= 0 && p + 1 < nnz);
        if (p < 0 || p + 1 >= nnz) return;
        dtci[(size_t)p] = c;
        dtci[(size_t)p + 1] = c + d;
        dtv[(size_t)p] = cs::value(g, w, c, nd);
        dtv[(size_t)p + 1] = cs::value(g, w, c + d, nd);
    }
    CHECK(same(hcol, dcol));
    CHECK(same(hval, dval));
    CHECK(same(htrp, dtrp));
    CHECK(same(htci, dtci));
    CHECK(same(htv, dtv));
    // ---- window pointers: the chosen width, and widths that cut the rows everywhere
    const int32_t wins[] = {window_width(nl, 2048), 1, 2, 3, 5, 7, 16, 37, 100};
    for (int32_t win : wins) {
        const int32_t nwin = (nl + win - 1) / win;
        std::vector<int32_t> hwp((size_t)(nwin + 1) * m), dwp((size_t)(nwin + 1) * m);
        window_pointers(m, rowptr.data(), hcol.data(), nl, win, nwin, hwp.data());
        for (int32_t t = 0; t < (nwin + 1) * m; ++t) dwp[(size_t)t] = cs::window_pointer(g, t % m, t / m, win);   // constraints_win_kernel
        CHECK(same(hwp, dwp));
    }
}

int main()
{
    for (int mx = 3; mx <= 10; ++mx)
        for (int my = 3; my <= 10; ++my)
            for (int u0 = 0; u0 <= my; ++u0)
                for (int u1 = u0; u1 <= my; ++u1) one_slab(mx, my, 0, u0, u1);
    for (int mx = 3; mx <= 6; ++mx)
        for (int my = 3; my <= 6; ++my)
            for (int mz = 3; mz <= 6; ++mz)
                for (int u0 = 0; u0 <= mz; ++u0)
                    for (int u1 = u0; u1 <= mz; ++u1) one_slab(mx, my, mz, u0, u1);
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    if (g_failed) return 1;
    std::printf("all constraints core checks passed\n");
    return 0;
}
