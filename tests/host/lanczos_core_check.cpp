// lanczos_core_check.cpp -- the scalar rule of -spk_amg_lanczos resident on the host (csrc/spk_lanczos_core.hpp: the state
// block and the transitions the kernels' finishing workgroup applies) without a GPU.  A plain Lanczos on D^-1/2 A D^-1/2 of
// small dense SPD matrices keeps its tridiagonal with push_back and break exactly as dev_lanczos (spk_amg_setup.cpp) does and
// records the two sums of every step; the same sums then go through the state machine for ALL kk steps -- behind the break
// with poison values, as the device enqueues every step blind -- and steps, al and be must agree byte for byte, the state
// behind the break untouched.  Compiled with g++ and the sanitizers by tests/test_amg_lanczos_cpu.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "spk_lanczos_core.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

namespace lz = spk::lanczos_core;

static double hashed(uint32_t i, uint32_t salt)   // in (-1, 1), full mantissas
{
    uint32_t h = i * 2654435761u + salt * 0x9e3779b9u + 12345u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    return (double)h / 2147483648.0 - 1.0;
}

struct Sums {
    double init = 0.0;
    std::vector<double> dot, upd;   // of the steps the loop ran
};

// dev_lanczos with a dense product: the kernels' passes as loops, the host's scalar sequence verbatim.  nan_at >= 0: the
// dot of that step comes back as NaN.
static void plain_lanczos(const std::vector<double> &A, int n, int nan_at, std::vector<double> &al, std::vector<double> &be, Sums &sm)
{
    std::vector<double> sv((size_t)n), q((size_t)n), qp((size_t)n, 0.0), w((size_t)n), t((size_t)n), aw((size_t)n);
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
        sv[(size_t)i] = std::sqrt(std::fabs(1.0 / A[(size_t)i * n + i]));
        uint32_t h = (uint32_t)i * 2654435761u + 0x9e3779b9u;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        const double x = 0.5 + (double)(h & 0xffffu) / 65536.0;
        q[(size_t)i] = x;
        acc += x * x;
    }
    sm.init = acc;
    const double nq = std::sqrt(acc);
    for (int i = 0; i < n; ++i) {
        q[(size_t)i] = q[(size_t)i] / nq;
        t[(size_t)i] = sv[(size_t)i] * q[(size_t)i];
    }
    al.clear();
    be.assign(1, 0.0);
    const int kk = std::min(lz::kSteps, n);
    std::vector<double> *qc = &q, *qo = &qp;
    for (int j = 0; j < kk; ++j) {
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int c = 0; c < n; ++c) s += A[(size_t)i * n + c] * t[(size_t)c];
            aw[(size_t)i] = s;
        }
        acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const double x = sv[(size_t)i] * aw[(size_t)i];
            w[(size_t)i] = x;
            acc += x * (*qc)[(size_t)i];
        }
        if (j == nan_at) acc = std::numeric_limits<double>::quiet_NaN();
        sm.dot.push_back(acc);
        const double a = acc;
        al.push_back(a);
        acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const double x = w[(size_t)i] - (a * (*qc)[(size_t)i] + be.back() * (*qo)[(size_t)i]);
            w[(size_t)i] = x;
            acc += x * x;
        }
        sm.upd.push_back(acc);
        const double nb = std::sqrt(acc);
        if (j + 1 == kk || nb <= 1e-12 * std::fabs(a)) break;
        be.push_back(nb);
        std::swap(qc, qo);
        for (int i = 0; i < n; ++i) {
            (*qc)[(size_t)i] = w[(size_t)i] / nb;
            t[(size_t)i] = sv[(size_t)i] * (*qc)[(size_t)i];
        }
    }
}

// the recorded sums through the state machine for all kk steps; behind the recorded ones poison
static void check_case(const char *name, const std::vector<double> &A, int n, int want_steps, int nan_at = -1)
{
    std::vector<double> al, be;
    Sums sm;
    plain_lanczos(A, n, nan_at, al, be, sm);
    const int kk = std::min(lz::kSteps, n);
    lz::LzState st, at_stop;
    std::memset(&st, 0, sizeof st);
    std::memset(&at_stop, 0, sizeof at_stop);
    lz::lz_after_init(&st, sm.init);
    bool seen_stop = false;
    for (int j = 0; j < kk; ++j) {
        const bool live = (size_t)j < sm.dot.size();
        lz::lz_after_dot(&st, j, live ? sm.dot[(size_t)j] : 1e300 + j);
        lz::lz_after_update(&st, j, kk, live ? sm.upd[(size_t)j] : 4.0 + j);
        if (!live) CHECK(std::memcmp(&st, &at_stop, sizeof st) == 0);   // behind the break nothing moves
        if (st.stopped && !seen_stop) {
            std::memcpy(&at_stop, &st, sizeof st);
            seen_stop = true;
            CHECK((size_t)j + 1 == sm.dot.size());   // the break of the loop, at its step
        }
    }
    const double nq = std::sqrt(sm.init);
    CHECK(std::memcmp(&st.nq, &nq, sizeof nq) == 0);
    CHECK(st.stopped == 1);
    CHECK(st.steps == (int32_t)al.size() && al.size() == be.size());
    CHECK(st.steps == want_steps);
    CHECK(std::memcmp(st.al, al.data(), sizeof(double) * al.size()) == 0);
    CHECK(std::memcmp(st.be, be.data(), sizeof(double) * be.size()) == 0);
    for (int j = st.steps; j < lz::kSteps; ++j) CHECK(st.al[j] == 0.0 && st.be[j] == 0.0);   // (as zeroed)
    std::printf("case %-22s n %2d kk %2d steps %2d al[0] %.17g\n", name, n, kk, (int)st.steps, st.al[0]);
}

static std::vector<double> dense_spd(int n, uint32_t salt)
{
    std::vector<double> A((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < i; ++c) A[(size_t)i * n + c] = A[(size_t)c * n + i] = hashed((uint32_t)(i * n + c), salt);
    for (int i = 0; i < n; ++i) A[(size_t)i * n + i] = (double)n + 1.0 + hashed((uint32_t)i, salt + 7u);   // strictly dominant
    return A;
}

int main()
{
    check_case("dense40", dense_spd(40, 1u), 40, 30);
    check_case("dense18", dense_spd(18, 2u), 18, 18);
    {   // D^-1 A = I: the first norm is zero
        const int n = 12;
        std::vector<double> A((size_t)n * n, 0.0);
        for (int i = 0; i < n; ++i) A[(size_t)i * n + i] = 1.0 + (double)(i % 5);
        check_case("diagonal", A, n, 1);
    }
    {   // D^-1/2 A D^-1/2 = blocks [[1, 1/2], [1/2, 1]] and ones: eigenvalues 1/2, 1, 3/2 -- the Krylov space ends at 3
        const int n = 14;
        std::vector<double> A((size_t)n * n, 0.0), d((size_t)n);
        for (int i = 0; i < n; ++i) d[(size_t)i] = (double)(1 << (2 * (i % 3)));   // 1, 4, 16: exact square roots
        for (int i = 0; i < n; ++i) A[(size_t)i * n + i] = d[(size_t)i];
        for (int i = 0; i + 1 < 8; i += 2)
            A[(size_t)i * n + i + 1] = A[(size_t)(i + 1) * n + i] = 0.5 * std::sqrt(d[(size_t)i]) * std::sqrt(d[(size_t)i + 1]);
        check_case("three eigenvalues", A, n, 3);
    }
    check_case("nan at step 2", dense_spd(40, 3u), 40, 30, 2);
    check_case("one row", dense_spd(1, 4u), 1, 1);
    if (failures) {
        std::printf("%d lanczos core check(s) FAILED\n", failures);
        return 1;
    }
    std::printf("all lanczos core checks passed\n");
    return 0;
}
