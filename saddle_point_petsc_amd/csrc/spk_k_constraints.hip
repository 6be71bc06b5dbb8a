// spk_k_constraints.hip -- the constraint block B of the reference's own discretisation (the mean and moment rows of
// SpkAssembleOperator_Constraints[3D]) written where KSPSetOperators consumes it: B by rows with localised columns,
// B^T by rows and the column-window pointers of a slab of whole node lines (2-D) or planes (3-D), in device memory, bit
// for bit what the host chain (generator, localise_and_sort, window_pointers, transpose_rows) uploads.
//
// Why the bits match: positions, columns and values are the closed forms of spk_constraints_core.hpp, which the CPU
// check (tests/host/constraints_core_check.cpp) runs against the host chain; the values are the generator's expressions
// in its order, compiled without contraction.  Every word is written once by the thread that owns it: no atomics.
//
//   constraints_b_kernel     one thread per interior node: its entry of each of the m rows (m coalesced store streams)
//   constraints_bt_kernel    one thread per local row of B^T: the row pointer, and the two entries of an interior node's row
//   constraints_win_kernel   one thread per (window, row)
#include "spk_internal.hpp"
#include "spk_constraints_core.hpp"

#pragma clang fp contract(off)

namespace spk {
namespace k {

namespace {

namespace cs = spk::constraints;
constexpr int kConThreads = 256;

__global__ __launch_bounds__(kConThreads) void constraints_b_kernel(cs::Slab g, int64_t nint, int32_t *__restrict__ colidx,
                                                                    double *__restrict__ val)
{
    const int64_t q = (int64_t)blockIdx.x * kConThreads + threadIdx.x;
    if (q >= nint) return;
    const cs::Node nd = cs::interior_node(g, q);
    const double w = cs::weight(g);
    const int m = cs::rows(g);
    for (int r = 0; r < m; ++r) {
        const int64_t p = (int64_t)r * nint + q;
        colidx[p] = cs::b_column(g, r, nd);
        val[p] = cs::value(g, w, r, nd);
    }
}

__global__ __launch_bounds__(kConThreads) void constraints_bt_kernel(cs::Slab g, int64_t nl, int32_t *__restrict__ rowptr,
                                                                     int32_t *__restrict__ colidx, double *__restrict__ val)
{
    const int64_t lr = (int64_t)blockIdx.x * kConThreads + threadIdx.x;
    if (lr > nl) return;
    const int64_t p = cs::bt_rowptr(g, lr);
    rowptr[lr] = (int32_t)p;
    if (lr == nl) return;
    const int d = cs::dof(g);
    const int64_t N = lr / d;
    const int c = (int)(lr - N * d);
    bool in;
    const cs::Node nd = cs::local_node(g, N, in);
    if (!in) return;
    const double w = cs::weight(g);
    colidx[p] = c;
    colidx[p + 1] = c + d;
    val[p] = cs::value(g, w, c, nd);
    val[p + 1] = cs::value(g, w, c + d, nd);
}

__global__ __launch_bounds__(kConThreads) void constraints_win_kernel(cs::Slab g, int32_t win, int32_t nwin, int32_t *__restrict__ winptr)
{
    const int m = cs::rows(g);
    const int t = (int)(blockIdx.x * kConThreads + threadIdx.x);
    if (t >= (nwin + 1) * m) return;
    winptr[t] = cs::window_pointer(g, t % m, t / m, win);
}

}  // namespace

void assemble_constraints(int mx, int my, int mz, int u0, int u1, int32_t *bcol, double *bval, int32_t *trp, int32_t *tci, double *tv,
                          int32_t win, int32_t nwin, int32_t *winptr, hipStream_t s)
{
    const cs::Slab g{mx, my, mz, u0, u1};
    const int64_t nint = cs::row_count(g), nl = cs::local_cols(g);
    const int64_t gb = (nint + kConThreads - 1) / kConThreads, gt = (nl + 1 + kConThreads - 1) / kConThreads;
    const int64_t gw = ((int64_t)(nwin + 1) * cs::rows(g) + kConThreads - 1) / kConThreads;
    if (gb > INT32_MAX || gt > INT32_MAX || gw > INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "device constraints: the launch grid");
    if (gb > 0) hipLaunchKernelGGL(constraints_b_kernel, dim3((unsigned)gb), dim3(kConThreads), 0, s, g, nint, bcol, bval);
    hipLaunchKernelGGL(constraints_bt_kernel, dim3((unsigned)gt), dim3(kConThreads), 0, s, g, nl, trp, tci, tv);
    hipLaunchKernelGGL(constraints_win_kernel, dim3((unsigned)gw), dim3(kConThreads), 0, s, g, win, nwin, winptr);
    SPK_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace spk
