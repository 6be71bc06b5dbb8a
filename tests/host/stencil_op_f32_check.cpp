// stencil_op_f32_check.cpp -- a row of a grid-stencil level operator in FP32 on the host (csrc/spk_stencil_op_core.hpp: so_row
// on float, what the kernels of -spk_mg_precision single run) without a GPU: on every node grid given on the command line
// (bs nx ny nz, repeated; without arguments a few small ones) the product and the smoothing step from the value array alone
// equal, byte for byte, a plain float loop over the row in stored order -- every product and every addition rounded to
// float on its own; every buffer has its exact size (the sanitizers watch every index).  Per grid it prints which residues
// mod 4 the begin and the end of the workgroups' value ranges take (so_wg_rows rows per workgroup): the kernel stages a
// range in 16-byte pieces of four floats and peels up to three values in front and behind.
// Compiled with g++ and the sanitizers by tests/test_mg_precision_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// values in (-1, 1) with full float mantissas from an integer hash: sums whose bits depend on their order
static float hashed(uint32_t i, uint32_t salt)
{
    uint32_t h = i * 2654435761u + salt * 0x9e3779b9u + 12345u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    return (float)((double)h / 2147483648.0 - 1.0);
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

template <int BS>
static void check_grid(int32_t nx, int32_t ny, int32_t nz)
{
    const int32_t nd[3] = {nx, ny, nz};
    const int32_t n = nx * ny * nz * BS;
    const int64_t nnz = gs::gs_nnz(nd, BS);
    std::vector<int32_t> rp((size_t)n + 1, -1), ci((size_t)nnz, -1);
    for (int32_t k = 0; k < nz; ++k)
        for (int32_t j = 0; j < ny; ++j)
            for (int32_t i = 0; i < nx; ++i)
                for (int a = 0; a < BS; ++a) {
                    const int32_t r = ((k * ny + j) * nx + i) * BS + a;
                    rp[(size_t)r] = (int32_t)gs::gs_row_offset(nd, BS, i, j, k, a);
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

    std::vector<float> v((size_t)nnz), x((size_t)n), xo((size_t)n), b((size_t)n), dinv((size_t)n);
    for (int64_t p = 0; p < nnz; ++p) v[(size_t)p] = hashed((uint32_t)p, 1);
    for (int32_t r = 0; r < n; ++r) {
        x[(size_t)r] = hashed((uint32_t)r, 2), xo[(size_t)r] = hashed((uint32_t)r, 3), b[(size_t)r] = hashed((uint32_t)r, 4);
        dinv[(size_t)r] = 0.5f + 0.25f * hashed((uint32_t)r, 5);
    }
    const float alpha = 0.7f, beta = 0.3f;
    for (int32_t r = 0; r < n; ++r) {
        // the plain float loop in stored order: the first product, then one rounded product and one addition per entry
        // (volatile: the product is stored as a float before it is added, whatever the compiler would like to fuse)
        float d = 0.0f;
        for (int32_t p = rp[(size_t)r]; p < rp[(size_t)r + 1]; ++p) {
            volatile float t = v[(size_t)p] * x[(size_t)ci[(size_t)p]];
            d = p == rp[(size_t)r] ? (float)t : d + t;
        }
        const float y = x[(size_t)r];
        volatile float q0 = b[(size_t)r] - d;
        volatile float q1 = dinv[(size_t)r] * q0;
        volatile float q2 = alpha * q1;
        const float s0 = y + q2;   // beta == 0
        volatile float q3 = beta * (y - 0.0f);
        const float s1 = s0 + q3;   // xo null
        volatile float q4 = y - xo[(size_t)r];
        volatile float q5 = beta * q4;
        const float s2 = s0 + q5;
        const so::SoRow w = so::so_row_of<BS>(nd, r);
        const float *vr = v.data() + rp[(size_t)r];
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
    // the workgroups' value ranges [begin, end) of the float launch, and of the double one for comparison
    const int32_t rows = so::so_wg_rows(nd, BS, (int32_t)sizeof(float));
    CHECK(rows >= 64 && rows <= 256 && rows % 64 == 0 && rows >= so::so_wg_rows(nd, BS, (int32_t)sizeof(double)));
    CHECK((int64_t)rows * so::so_max_row(nd, BS) * (int64_t)sizeof(float) <= 32768 || rows == 64);
    bool begin[4] = {false, false, false, false}, end[4] = {false, false, false, false};
    int32_t groups = 0;
    for (int32_t r0 = 0; r0 < n; r0 += rows, ++groups) {
        const int32_t r1 = r0 + rows < n ? r0 + rows : n;
        const int64_t p0 = so::so_row_begin<BS>(nd, r0), p1 = so::so_row_begin<BS>(nd, r1);
        CHECK(p0 == rp[(size_t)r0] && p1 == rp[(size_t)r1] && p0 % BS == 0 && p1 - p0 <= (int64_t)rows * so::so_max_row(nd, BS));
        begin[p0 & 3] = true, end[p1 & 3] = true;
    }
    std::printf("grid %d x %d x %d, bs %d: %d rows, %lld entries, %d workgroups of %d rows, begin residues mod 4:", (int)nx, (int)ny,
                (int)nz, BS, (int)n, (long long)nnz, (int)groups, (int)rows);
    for (int q = 0; q < 4; ++q) if (begin[q]) std::printf(" %d", q);
    std::printf(", end residues mod 4:");
    for (int q = 0; q < 4; ++q) if (end[q]) std::printf(" %d", q);
    std::printf("\n");
}

static void check(int bs, int32_t nx, int32_t ny, int32_t nz)
{
    if (bs == 1) check_grid<1>(nx, ny, nz);
    else if (bs == 2) check_grid<2>(nx, ny, nz);
    else if (bs == 3) check_grid<3>(nx, ny, nz);
    else CHECK(bs >= 1 && bs <= 3);
}

int main(int argc, char **argv)
{
    if ((argc - 1) % 4 != 0) {
        std::printf("usage: %s [bs nx ny nz]...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 3 < argc; a += 4) check(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2]), std::atoi(argv[a + 3]));
    if (argc == 1) {
        const int32_t flat[4][2] = {{3, 3}, {2, 2}, {17, 9}, {9, 1}};
        for (const auto &g : flat)
            for (int bs = 1; bs <= 3; ++bs) check(bs, g[0], g[1], 1);
        check(3, 5, 5, 3);
        check(3, 3, 2, 2);
    }
    if (failures) {
        std::printf("%d FP32 stencil operator host checks FAILED\n", failures);
        return 1;
    }
    std::printf("all FP32 stencil operator host checks passed\n");
    return 0;
}
