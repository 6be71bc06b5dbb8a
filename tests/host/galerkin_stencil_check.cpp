// galerkin_stencil_check.cpp -- the grid-stencil Galerkin product on the host (csrc/spk_galerkin_core.hpp through
// csrc/spk_galerkin_host.cpp: galerkin_stencil_host, galerkin_stencil_check_host, galerkin_stencil_children) without a GPU: the
// closed-form pattern, bitwise symmetry, the values against a dense P^T A P under a symmetric and a non-symmetric value rule,
// the buffers' exact sizes (the sanitizers watch every index) and the level-0 refusal.  Compiled with g++ and the sanitizers by tests/test_mg_galerkin_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "spk_galerkin_core.hpp"
#include "spk_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

namespace gs = spk::galerkin;

struct Csr {
    std::vector<int32_t> rp{0}, ci;
    std::vector<double> v;
};

// an operator with full bs x bs blocks on the 3^d stencil (corners = false: on the 2 d + 1 point stencil), values from a
// fixed recurrence.  symmetric = false: val(r, c) != val(c, r), so that the symmetrisation averages two different numbers
// and a gather that reads the transposed slot or the transposed block gives other values
static Csr stencil_operator(const int32_t d[3], int bs, bool corners, bool symmetric = true)
{
    auto val = [symmetric](int64_t r, int64_t c) {
        const int64_t lo = !symmetric || r < c ? r : c, hi = !symmetric || r < c ? c : r;
        const double x = (double)((lo * 7919 + hi * 104729) % 1009) / 1009.0;
        return r == c ? 30.0 + x : -(0.25 + x);
    };
    Csr A;
    for (int32_t k = 0; k < d[2]; ++k)
        for (int32_t j = 0; j < d[1]; ++j)
            for (int32_t i = 0; i < d[0]; ++i)
                for (int a = 0; a < bs; ++a) {
                    const int64_t r = ((int64_t)(k * d[1] + j) * d[0] + i) * bs + a;
                    for (int32_t k2 = k - 1; k2 <= k + 1; ++k2)
                        for (int32_t j2 = j - 1; j2 <= j + 1; ++j2)
                            for (int32_t i2 = i - 1; i2 <= i + 1; ++i2) {
                                if (i2 < 0 || i2 >= d[0] || j2 < 0 || j2 >= d[1] || k2 < 0 || k2 >= d[2]) continue;
                                if (!corners && (i2 != i) + (j2 != j) + (k2 != k) > 1) continue;
                                for (int b = 0; b < bs; ++b) {
                                    const int64_t c = ((int64_t)(k2 * d[1] + j2) * d[0] + i2) * bs + b;
                                    A.ci.push_back((int32_t)c);
                                    A.v.push_back(val(r, c));
                                }
                            }
                    A.rp.push_back((int32_t)A.ci.size());
                }
    return A;
}

static void run(const int32_t fd[3], const int32_t cd[3], int bs, bool corners, bool symmetric)
{
    const Csr A = stencil_operator(fd, bs, corners, symmetric);
    if (!symmetric) {   // the rule does what it is for: some pair of the first node's entries differs
        bool differs = false;
        for (int32_t q = A.rp[0]; q < A.rp[1]; ++q) {
            const int32_t c = A.ci[(size_t)q];
            for (int32_t t = A.rp[(size_t)c]; t < A.rp[(size_t)c + 1]; ++t)
                if (A.ci[(size_t)t] == 0 && A.v[(size_t)t] != A.v[(size_t)q]) differs = true;
        }
        CHECK(differs);
    }
    const int64_t nf = (int64_t)fd[0] * fd[1] * fd[2] * bs, nc = (int64_t)cd[0] * cd[1] * cd[2] * bs, nz = gs::gs_nnz(cd, bs);
    spk::galerkin_stencil_check_host(fd, bs, A.rp.data(), A.ci.data());
    std::vector<int32_t> rp((size_t)nc + 1, -1), ci((size_t)nz, -1);   // exactly as long as the closed form says
    std::vector<double> v((size_t)nz, NAN);
    spk::galerkin_stencil_host(fd, cd, bs, A.rp.data(), A.ci.data(), A.v.data(), rp.data(), ci.data(), v.data());
    // the pattern: clipped 3^d neighbourhood, full blocks, ascending; every slot written
    int64_t p = 0;
    for (int32_t k = 0; k < cd[2]; ++k)
        for (int32_t j = 0; j < cd[1]; ++j)
            for (int32_t i = 0; i < cd[0]; ++i)
                for (int a = 0; a < bs; ++a) {
                    CHECK(rp[(size_t)(((int64_t)(k * cd[1] + j) * cd[0] + i) * bs + a)] == p);
                    for (int32_t k2 = k - 1; k2 <= k + 1; ++k2)
                        for (int32_t j2 = j - 1; j2 <= j + 1; ++j2)
                            for (int32_t i2 = i - 1; i2 <= i + 1; ++i2) {
                                if (i2 < 0 || i2 >= cd[0] || j2 < 0 || j2 >= cd[1] || k2 < 0 || k2 >= cd[2]) continue;
                                for (int b = 0; b < bs; ++b, ++p) {
                                    CHECK(ci[(size_t)p] == ((k2 * cd[1] + j2) * cd[0] + i2) * bs + b);
                                    CHECK(p == gs::gs_pos(cd, bs, i, j, k, a, i2, j2, k2, b));
                                }
                            }
                }
    CHECK(p == nz && rp[(size_t)nc] == nz);
    // dense P from the children, then (P^T A P + its transpose) / 2
    std::vector<double> P((size_t)(nf * nc), 0.0), AP((size_t)(nf * nc), 0.0), aAP((size_t)(nf * nc), 0.0), G((size_t)(nc * nc), 0.0),
        T((size_t)(nc * nc), 0.0);   // T = |P|^T |A| |P|
    std::vector<double> colsum((size_t)(nf / bs), 0.0);
    for (int32_t C = 0; C < nc / bs; ++C) {
        int32_t nodes[27];
        double w[27];
        const int n = spk::galerkin_stencil_children(fd, cd, C, nodes, w);
        CHECK(n >= 1 && n <= 27);
        for (int q = 0; q < n; ++q) {
            CHECK(q == 0 || nodes[q] > nodes[q - 1]);
            colsum[(size_t)nodes[q]] += w[q];
            for (int a = 0; a < bs; ++a) P[(size_t)(((int64_t)nodes[q] * bs + a) * nc + (int64_t)C * bs + a)] = w[q];
        }
    }
    for (double s : colsum) CHECK(s == 1.0);   // every fine node interpolates a constant exactly
    for (int64_t r = 0; r < nf; ++r)
        for (int32_t q = A.rp[(size_t)r]; q < A.rp[(size_t)r + 1]; ++q)
            for (int64_t c = 0; c < nc; ++c) {
                AP[(size_t)(r * nc + c)] += A.v[(size_t)q] * P[(size_t)((int64_t)A.ci[(size_t)q] * nc + c)];
                aAP[(size_t)(r * nc + c)] += std::fabs(A.v[(size_t)q]) * P[(size_t)((int64_t)A.ci[(size_t)q] * nc + c)];
            }
    for (int64_t r = 0; r < nf; ++r)
        for (int64_t a = 0; a < nc; ++a) {
            const double w = P[(size_t)(r * nc + a)];
            if (w == 0.0) continue;
            for (int64_t c = 0; c < nc; ++c) {
                G[(size_t)(a * nc + c)] += w * AP[(size_t)(r * nc + c)];
                T[(size_t)(a * nc + c)] += w * aAP[(size_t)(r * nc + c)];
            }
        }
    std::vector<double> N((size_t)(nc * nc), 0.0);
    for (int64_t r = 0; r < nc; ++r)
        for (int32_t q = rp[(size_t)r]; q < rp[(size_t)r + 1]; ++q) N[(size_t)(r * nc + ci[(size_t)q])] = v[(size_t)q];
    const double eps = std::ldexp(1.0, -53), nine_d = fd[2] > 1 ? 729.0 : 81.0;
    for (int64_t r = 0; r < nc; ++r)
        for (int64_t c = 0; c < nc; ++c) {
            const double got = N[(size_t)(r * nc + c)], ref = 0.5 * (G[(size_t)(r * nc + c)] + G[(size_t)(c * nc + r)]);
            const double bound = 2.0 * nine_d * eps * 0.5 * (T[(size_t)(r * nc + c)] + T[(size_t)(c * nc + r)]);
            CHECK(std::fabs(got - ref) <= bound);
            CHECK(std::memcmp(&got, &N[(size_t)(c * nc + r)], sizeof got) == 0);   // bitwise symmetric
        }
}

int main()
{
    for (const bool symmetric : {true, false}) {   // every grid under both value rules
        const int32_t a5[3] = {5, 5, 1}, a3[3] = {3, 3, 1};
        run(a5, a3, 2, true, symmetric);     // one interior coarse node
        const int32_t b0[3] = {12, 10, 1}, b1[3] = {7, 6, 1}, b2[3] = {4, 4, 1}, b3[3] = {3, 3, 1};
        run(b0, b1, 2, true, symmetric);     // both sides even: the single-child last node
        run(b1, b2, 2, true, symmetric);     // odd x, even y
        run(b2, b3, 1, false, symmetric);    // 4 -> 3, a 5-point operator
        const int32_t c0[3] = {12, 9, 1}, c1[3] = {12, 5, 1};
        run(c0, c1, 1, false, symmetric);    // x does not halve
        const int32_t d0[3] = {6, 4, 3}, d1[3] = {4, 3, 3};
        run(d0, d1, 3, true, symmetric);     // 3-D, z does not halve
        const int32_t e0[3] = {5, 5, 5}, e1[3] = {3, 3, 3};
        run(e0, e1, 3, true, symmetric);
    }
    // the refusal: an entry two nodes away in x
    {
        const int32_t fd[3] = {6, 4, 1};
        Csr A = stencil_operator(fd, 1, false);
        std::vector<int32_t> ci = A.ci;
        ci[(size_t)A.rp[9] - 1] = 11;   // row 8 = node (2, 1): its last column becomes node (5, 1)
        bool threw = false;
        try {
            spk::galerkin_stencil_check_host(fd, 1, A.rp.data(), ci.data());
        } catch (const spk::Error &e) {
            threw = e.code == SPK_ERR_UNSUPPORTED && e.msg.find("row 8, column 11") != std::string::npos &&
                    e.msg.find("-spk_mg_galerkin products") != std::string::npos;
        }
        CHECK(threw);
    }
    if (failures) {
        std::printf("%d galerkin stencil host checks FAILED\n", failures);
        return 1;
    }
    std::printf("all galerkin stencil host checks passed\n");
    return 0;
}
