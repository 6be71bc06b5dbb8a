// stencil_op_check.cpp -- a row of a grid-stencil level operator on the host (csrc/spk_stencil_op_core.hpp: so_row, the one
// function the kernels of -spk_mg_operator stencil run) without a GPU: for node grids with corner, edge and interior rows,
// one-plane and 3-D, every node size, the product and the smoothing step from the value array alone equal, byte for byte,
// a plain CSR loop in stored order over the pattern the gs_* functions give; every buffer has its exact size (the
// sanitizers watch every index).  Compiled with g++ and the sanitizers by tests/test_mg_operator_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "spk_stencil_op_core.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

namespace gs = spk::galerkin;
namespace so = spk::stencil_op;

// values in (-1, 1) with full mantissas from an integer hash: sums whose bits depend on their order
static double hashed(uint32_t i, uint32_t salt)
{
    uint32_t h = i * 2654435761u + salt * 0x9e3779b9u + 12345u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    uint32_t g = h * 747796405u + 2891336453u;
    g ^= g >> 17;
    return ((double)h + (double)g / 4294967296.0) / 2147483648.0 - 1.0;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

template <int BS>
static void check_grid(int32_t nx, int32_t ny, int32_t nz)
{
    const int32_t nd[3] = {nx, ny, nz};
    const int32_t n = nx * ny * nz * BS;
    const int64_t nnz = gs::gs_nnz(nd, BS);
    // the pattern from the gs_* functions: every entry placed by gs_pos, the row pointers by gs_row_offset
    std::vector<int32_t> rp((size_t)n + 1, -1), ci((size_t)nnz, -1);
    for (int32_t k = 0; k < nz; ++k)
        for (int32_t j = 0; j < ny; ++j)
            for (int32_t i = 0; i < nx; ++i)
                for (int a = 0; a < BS; ++a) {
                    const int32_t r = ((k * ny + j) * nx + i) * BS + a;
                    rp[(size_t)r] = (int32_t)gs::gs_row_offset(nd, BS, i, j, k, a);
                    CHECK(so::so_row_begin<BS>(nd, r) == rp[(size_t)r]);
                    const so::SoRow w = so::so_row_of<BS>(nd, r);
                    CHECK(w.i == i && w.j == j && w.k == k && w.a == a);
                    for (int32_t k2 = gs::gs_first(k); k2 < gs::gs_first(k) + gs::gs_width(k, nz); ++k2)
                        for (int32_t j2 = gs::gs_first(j); j2 < gs::gs_first(j) + gs::gs_width(j, ny); ++j2)
                            for (int32_t i2 = gs::gs_first(i); i2 < gs::gs_first(i) + gs::gs_width(i, nx); ++i2)
                                for (int b = 0; b < BS; ++b) {
                                    const int64_t p = gs::gs_pos(nd, BS, i, j, k, a, i2, j2, k2, b);
                                    CHECK(p >= 0 && p < nnz && ci[(size_t)p] == -1);
                                    if (p >= 0 && p < nnz) ci[(size_t)p] = ((k2 * ny + j2) * nx + i2) * BS + b;
                                }
                }
    rp[(size_t)n] = (int32_t)nnz;
    CHECK(so::so_row_begin<BS>(nd, n) == nnz);
    int32_t longest = 0;
    for (int32_t r = 0; r < n; ++r) {
        CHECK(rp[(size_t)r] < rp[(size_t)r + 1]);
        longest = rp[(size_t)r + 1] - rp[(size_t)r] > longest ? rp[(size_t)r + 1] - rp[(size_t)r] : longest;
        for (int32_t p = rp[(size_t)r]; p < rp[(size_t)r + 1]; ++p) {
            CHECK(ci[(size_t)p] >= 0 && ci[(size_t)p] < n);
            if (p > rp[(size_t)r]) CHECK(ci[(size_t)p] > ci[(size_t)p - 1]);
        }
    }
    CHECK(longest == so::so_max_row(nd, BS));

    std::vector<double> v((size_t)nnz), x((size_t)n), xo((size_t)n), b((size_t)n), dinv((size_t)n);
    for (int64_t p = 0; p < nnz; ++p) v[(size_t)p] = hashed((uint32_t)p, 1);
    for (int32_t r = 0; r < n; ++r) {
        x[(size_t)r] = hashed((uint32_t)r, 2), xo[(size_t)r] = hashed((uint32_t)r, 3), b[(size_t)r] = hashed((uint32_t)r, 4);
        dinv[(size_t)r] = 0.5 + 0.25 * hashed((uint32_t)r, 5);
    }
    const double alpha = 0.7, beta = 0.3;
    for (int32_t r = 0; r < n; ++r) {
        // the plain CSR loop in stored order: the first product, then one rounded product and one addition per entry
        double d = 0.0;
        for (int32_t p = rp[(size_t)r]; p < rp[(size_t)r + 1]; ++p) {
            const double t = v[(size_t)p] * x[(size_t)ci[(size_t)p]];
            d = p == rp[(size_t)r] ? t : d + t;
        }
        const double y = x[(size_t)r];
        const double s0 = y + alpha * (dinv[(size_t)r] * (b[(size_t)r] - d));   // beta == 0
        const double s1 = s0 + beta * (y - 0.0);                                // xo null
        const double s2 = s0 + beta * (y - xo[(size_t)r]);
        const so::SoRow w = so::so_row_of<BS>(nd, r);
        const double *vr = v.data() + rp[(size_t)r];
        CHECK(same_bits((so::so_row<BS, 0>(nd, w, vr, x.data(), nullptr, nullptr, nullptr, 0.0, 0.0)), d));
        CHECK(same_bits((so::so_row<BS, 1>(nd, w, vr, x.data(), dinv.data(), b.data(), nullptr, alpha, 0.0)), s0));
        CHECK(same_bits((so::so_row<BS, 1>(nd, w, vr, x.data(), dinv.data(), b.data(), xo.data(), alpha, 0.0)), s0));
        CHECK(same_bits((so::so_row<BS, 1>(nd, w, vr, x.data(), dinv.data(), b.data(), nullptr, alpha, beta)), s1));
        CHECK(same_bits((so::so_row<BS, 1>(nd, w, vr, x.data(), dinv.data(), b.data(), xo.data(), alpha, beta)), s2));
        // the lines whose loads are grouped change no bit
        CHECK(same_bits((so::so_row<BS, 0, 1>(nd, w, vr, x.data(), nullptr, nullptr, nullptr, 0.0, 0.0)), d));
        CHECK(same_bits((so::so_row<BS, 0, 3>(nd, w, vr, x.data(), nullptr, nullptr, nullptr, 0.0, 0.0)), d));
        CHECK(same_bits((so::so_row<BS, 1, 1>(nd, w, vr, x.data(), dinv.data(), b.data(), xo.data(), alpha, beta)), s2));
        CHECK(same_bits((so::so_row<BS, 1, 3>(nd, w, vr, x.data(), dinv.data(), b.data(), xo.data(), alpha, beta)), s2));
    }
    std::printf("grid %d x %d x %d, bs %d: %d rows, %lld entries, longest row %d\n", (int)nx, (int)ny, (int)nz, BS, (int)n,
                (long long)nnz, (int)longest);
}

int main()
{
    const int32_t flat[4][2] = {{3, 3}, {2, 2}, {17, 9}, {9, 1}};
    for (const auto &g : flat) {
        check_grid<1>(g[0], g[1], 1);
        check_grid<2>(g[0], g[1], 1);
        check_grid<3>(g[0], g[1], 1);
    }
    check_grid<3>(5, 5, 3);
    check_grid<3>(3, 2, 2);
    if (failures) {
        std::printf("%d stencil operator host checks FAILED\n", failures);
        return 1;
    }
    std::printf("all stencil operator host checks passed\n");
    return 0;
}
