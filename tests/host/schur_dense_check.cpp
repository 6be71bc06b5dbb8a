// schur_dense_check.cpp -- the host-pure step of the dense Schur complement (csrc/spk_host.cpp: schur_dense_factor)
// against brute force, without a GPU: compiled with g++ and the sanitizers by tests/test_schur_dense_host_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spk_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static double rnd(unsigned &s)
{
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / (double)(1u << 24) - 0.5;
}

int main()
{
    unsigned seed = 12345u;
    for (int m = 1; m <= 8; ++m) {
        // G = R R^T + a little asymmetry, as two orders of summation leave it
        std::vector<double> R((size_t)m * (m + 3)), G((size_t)m * m), S((size_t)m * m, -1.0), L((size_t)m * m, -1.0);
        for (double &v : R) v = rnd(seed);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) {
                double s = 0.0;
                for (int k = 0; k < m + 3; ++k) s += R[(size_t)i * (m + 3) + k] * R[(size_t)j * (m + 3) + k];
                G[(size_t)i * m + j] = s * (1.0 + (i < j ? 1e-15 : 0.0));
            }
        CHECK(spk::schur_dense_factor(m, G.data(), S.data(), L.data()) == -1);
        double err = 0.0, scale = 0.0;
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) {
                CHECK(S[(size_t)i * m + j] == S[(size_t)j * m + i]);
                CHECK(S[(size_t)i * m + j] == 0.5 * (G[(size_t)i * m + j] + G[(size_t)j * m + i]));
                if (j > i) CHECK(L[(size_t)i * m + j] == 0.0);
                double s = 0.0;
                for (int k = 0; k < m; ++k) s += L[(size_t)i * m + k] * L[(size_t)j * m + k];
                err = std::fmax(err, std::fabs(s - S[(size_t)i * m + j]));
                scale = std::fmax(scale, std::fabs(S[(size_t)i * m + j]));
            }
        CHECK(err <= 1e-14 * scale);
        if (m < 2) continue;
        // a repeated row: singular to working precision, refused at the pivot of the copy
        std::vector<double> D = G;
        for (int j = 0; j < m; ++j) D[(size_t)(m - 1) * m + j] = G[(size_t)0 * m + j], D[(size_t)j * m + (m - 1)] = G[(size_t)j * m + 0];
        D[(size_t)(m - 1) * m + (m - 1)] = G[0];
        CHECK(spk::schur_dense_factor(m, D.data(), S.data(), L.data()) == m - 1);
        // indefinite
        D = G;
        D[(size_t)1 * m + 1] = -D[(size_t)1 * m + 1];
        CHECK(spk::schur_dense_factor(m, D.data(), S.data(), L.data()) == 1);
    }
    if (failures) return 1;
    std::printf("all dense Schur host checks passed\n");
    return 0;
}
