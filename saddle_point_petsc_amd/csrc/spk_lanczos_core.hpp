// spk_lanczos_core.hpp -- the one source of the scalar rule of the device set-up's Lanczos under -spk_amg_lanczos resident
// (SPK_AMG_LANCZOS_RESIDENT): the state block that stays on the device and the transitions its sums take.  The kernels
// (spk_k_amg_setup.hip: thread 0 of the workgroup that finishes a sum) and the CPU run (tests/host/lanczos_core_check.cpp)
// call the same functions, so the block holds what the host loop of dev_lanczos (spk_amg_setup.cpp) would have kept because the
// same expressions ran on the same sums.  Standard library only; no ROCm.
//
// The host loop, for kk = min(kSteps, n) steps:
//     nq = sqrt(q.q);                                            be = {0}
//     step j:  a = w.q;  al.push_back(a);                        (the dot)
//              nb = sqrt(w.w);                                   (the update)
//              if (j + 1 == kk || nb <= 1e-12 * fabs(a)) break;
//              be.push_back(nb);
// The block: al[j] and be[j + 1] are the values pushed, steps = al.size(), stopped = the break was taken.  Once stopped,
// no transition changes anything, and every vector kernel of the route returns at its entry: the host enqueues all kk
// steps blind.  A NaN sum makes the comparison false, as in the loop: no stop.
// The square root is correctly rounded on both sides (std::sqrt; __dsqrt_rn), so the bits agree.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef SPK_HD
#ifdef __HIPCC__
#define SPK_HD __host__ __device__
#else
#define SPK_HD
#endif
#endif

namespace spk {
namespace lanczos_core {

constexpr int kSteps = 30;   // kLanczosSteps of spk_amg_levels.hpp

struct LzState {
    double al[kSteps];       // the diagonal: al[j] = the dot of step j
    double be[kSteps + 1];   // the off-diagonal: be[0] = 0, be[j + 1] = the norm that step j left
    double nq;               // the norm of the start vector
    int32_t steps;           // al[0 .. steps) and be[0 .. steps) are the tridiagonal
    int32_t stopped;         // the break rule has fired: nothing changes any more
};

SPK_HD inline double lz_sqrt(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(x);
#else
    return std::sqrt(x);
#endif
}

// after the init: sum = q.q
SPK_HD inline void lz_after_init(LzState *st, double sum) { st->nq = lz_sqrt(sum); }

// after the dot of step j: sum = w.q
SPK_HD inline void lz_after_dot(LzState *st, int j, double sum)
{
    if (st->stopped) return;
    st->al[j] = sum;
    st->steps = j + 1;
}

// after the update of step j of kk: sum = w.w
SPK_HD inline void lz_after_update(LzState *st, int j, int kk, double sum)
{
    if (st->stopped) return;
    const double nb = lz_sqrt(sum);
    if (j + 1 == kk || nb <= 1e-12 * std::fabs(st->al[j])) st->stopped = 1;
    else st->be[j + 1] = nb;
}

}  // namespace lanczos_core
}  // namespace spk
