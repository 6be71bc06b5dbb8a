// spk_amg_levels.hpp -- the multigrid set-up, stated once: the two loops over the levels (build_levels; with reuse on,
// refresh_levels) as templates over a route, and what both routes -- HostRoute (spk_amg_host.cpp: on the host, then
// uploaded; the default) and DevRoute (spk_amg_setup.cpp: on the device, -spk_gamg_setup device) -- take from the host
// unit.  Host-pure like spk_amg.hpp: the standard library and the project's host-pure headers only.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "spk_amg.hpp"
#include "spk_host.hpp"

namespace spk {

// ---- from spk_amg_host.cpp, where each is described ------------------------------------------------------------------
constexpr int kLanczosSteps = 30;
void sort_rows(HostCsr &A, std::vector<int32_t> *perm = nullptr);
int detect_bs(const HostCsr &A);
std::vector<double> diag_inv(const HostCsr &A);
void lanczos(const HostCsr &A, const std::vector<double> &dinv, double *lmin, double *lmax, double a_scale = 1.0);
void ritz_extremes(const std::vector<double> &al, const std::vector<double> &be, double *lmin, double *lmax);
int32_t aggregate(const std::vector<int32_t> &gp, const std::vector<int32_t> &gi, std::vector<int32_t> &agg);
bool grid_coarse_dims(const int32_t fd[3], int32_t cd[3], int sides);
int64_t grid_prolong_nnz(const int32_t fd[3], const int32_t cd[3], int bs);
std::vector<double> coarse_inverse(const HostCsr &A, double a_scale = 1.0);
double abs_sum(const std::vector<double> &x);
double binade_scale(double built, double now);
void smoother_interval(const spk_amg_opts &o, int l, double lmin, double lmax, double *lo, double *hi);
void smoother_coeffs(const spk_amg_opts &o, double lo, double hi, std::vector<double> &alpha, std::vector<double> &beta);
void fill_cycle_info(const spk_amg_opts &o, spk_amg_info &info);
void csr_out(const HostCsr &M, const CsrOut &o);
void coarse_inv_out(int32_t n, const double *cinv, const CsrOut &o);
void check_level_query(int L, int l, int which);
template <class Levels>   // of AmgLevel or AmgLevelDev: both keep `agg`
void aggregates_out(const Levels &lv, const spk_amg_info &info, int l, int32_t *nnodes, int32_t *agg)
{
    if (info.coarsening == SPK_AMG_COARSEN_GRID)
        fail(SPK_ERR_UNSUPPORTED, "amg: a grid-coarsened hierarchy has no aggregates (its levels are the node grids of spk_amg_info.dims)");
    if (l < 0 || l + 1 >= (int)lv.size()) fail(SPK_ERR_ARG, "amg: level %d has no aggregates", l);
    const std::vector<int32_t> &a = lv[(size_t)l].agg;
    if (nnodes) *nnodes = (int32_t)a.size();
    if (agg) std::memcpy(agg, a.data(), sizeof(int32_t) * a.size());
}

using Clock = std::chrono::steady_clock;
inline double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// The set-up, stated once: the level loop with every rule of the algorithm and the whole of `info`.  A route supplies
// what differs between the host and the device -- where the matrices live and what computes them:
//   rows(l), nnz(l) of A_l;  graph(l, bs, theta, gp, gi): the strong-connection graph of its nodes, in host vectors
//   ritz(l, &lmin, &lmax): the extreme Ritz values of D^-1 A_l (a level has its D^-1 from when it is appended)
//   set_interval(l, lo, hi): keeps what the smoother of level l needs
//   coarsen(l, bs, agg, na, omega, nsmooths): keeps agg; tentative P, nsmooths times P <- (I - omega D^-1 A) P, R = P^T;
//                                             appends level l+1 with A = (RAP + (RAP)^T) / 2 and its D^-1
//   coarsen_grid(l, bs, fd, cd): grid coarsening's step -- P of the node grids fd -> cd (no aggregates, no smoothing),
//                                             then R and level l+1 as coarsen has them
//   coarsest(): the last operator as a HostCsr;  set_coarse_inverse(x): keeps its dense inverse
// t0: when the caller began (its own preparation counts into info.setup_seconds).
template <class Route>
void build_levels(Route &r, int bs, const spk_amg_opts &o, int setup, Clock::time_point t0, spk_amg_info &info)
{
    if (r.rows(0) % bs) fail(SPK_ERR_ARG, "amg: block_size %d does not divide %d rows", bs, (int)r.rows(0));
    std::memset(&info, 0, sizeof info);
    const bool grid = o.coarsening == SPK_AMG_COARSEN_GRID;
    int32_t fd[3] = {o.grid[0], o.grid[1], o.grid[2]}, cd[3] = {0, 0, 0};
    if (grid && (int64_t)bs * fd[0] * fd[1] * fd[2] != (int64_t)r.rows(0))
        fail(SPK_ERR_ARG, "amg: grid coarsening: the operator has %d rows, the grid %d x %d x %d nodes of %d unknowns has %lld",
             (int)r.rows(0), (int)fd[0], (int)fd[1], (int)fd[2], bs, (long long)bs * fd[0] * fd[1] * fd[2]);
    bool stuck = false;   // grid coarsening: no direction halves any more
    double tot = 0.0;
    int l = 0;
    for (;; ++l) {
        const int32_t n = r.rows(l);
        info.rows[l] = n;
        info.nnz[l] = r.nnz(l);
        if (grid) std::memcpy(info.dims[l], fd, sizeof fd);
        tot += (double)info.nnz[l];
        if (n <= o.coarse_eq_limit || l + 1 == o.max_levels) break;
        // whether anything coarsens, before any Ritz call.  The grid is known: no graph, no aggregation
        std::vector<int32_t> gp, gi, agg;
        int32_t na = 0;
        if (grid) {
            if (!grid_coarse_dims(fd, cd, o.sides)) { stuck = true; break; }
        } else {
            r.graph(l, bs, o.threshold, gp, gi);
            na = aggregate(gp, gi, agg);
            if (na == 0 || (int64_t)na * bs >= n) break;   // no coarsening left
        }
        double lmin = 0.0, lmax = 0.0, lo = 0.0, hi = 0.0;
        r.ritz(l, &lmin, &lmax);
        info.lambda_max[l] = lmax;
        smoother_interval(o, l, lmin, lmax, &lo, &hi);
        r.set_interval(l, lo, hi);
        if (grid) {   // no prolongator smoothing either
            r.coarsen_grid(l, bs, fd, cd);
            std::memcpy(fd, cd, sizeof fd);
        } else {
            r.coarsen(l, bs, std::move(agg), na, 4.0 / (3.0 * lmax), o.nsmooths);
        }
    }
    info.levels = l + 1;
    info.coarsening = o.coarsening;
    info.sides = grid ? o.sides : 0;
    info.galerkin = grid ? o.galerkin : 0;
    if (r.rows(l) > SPK_AMG_MAX_COARSE && stuck) {   // (SPK_AMG_SIDES_ODD only: under ANY no side above 3 nodes is stuck)
        int a = 0;   // the largest side that does not halve
        for (int b = 1; b < 3; ++b) if (fd[b] > fd[a]) a = b;
        fail(SPK_ERR_UNSUPPORTED, "amg: the coarsest level keeps %d equations after %d levels; the dense coarse solve takes at "
             "most %d -- grid coarsening stops at %d x %d x %d nodes: the side of %d nodes (direction %c) cannot be halved "
             "(a side halves while it is odd and >= 5; sides of c 2^k + 1 nodes coarsen to the end) "
             "(`-spk_mg_sides any` coarsens even sides)", (int)r.rows(l), info.levels,
             SPK_AMG_MAX_COARSE, (int)fd[0], (int)fd[1], (int)fd[2], (int)fd[a], "xyz"[a]);
    }
    if (r.rows(l) > SPK_AMG_MAX_COARSE)
        fail(SPK_ERR_UNSUPPORTED, "amg: the coarsest level keeps %d equations after %d levels; the dense coarse solve takes at "
             "most %d -- raise -pc_mg_levels or -pc_gamg_threshold 0", (int)r.rows(l), info.levels, SPK_AMG_MAX_COARSE);
    r.set_coarse_inverse(coarse_inverse(r.coarsest()));
    info.block_size = bs;
    info.operator_complexity = tot / (double)std::max<int64_t>(info.nnz[0], 1);
    info.setup = setup;
    info.setup_seconds = seconds_since(t0);
}

// The refresh (spk_pc_set_amg_reuse), stated once: new values in A_0 and its D^-1, everything that was decided from the old
// ones kept -- the aggregates, P_tent, P_l (with the omega that smoothed it), R_l and every pattern.  Per level the Ritz
// values and the interval by the build's rule, then
//   regalerkin(l): A_{l+1} = (R A_l P + (R A_l P)^T) / 2 on its pattern, and its D^-1
// a_scale: the power of two by which the route's Lanczos and the coarse Cholesky see every A_l scaled (binade_scale)
// and at the end the coarse inverse.  levels(): of the kept hierarchy; check(): throws when a kernel reported an error.
// A throw leaves the hierarchy half-refreshed: the caller drops it.
template <class Route>
void refresh_levels(Route &r, const spk_amg_opts &o, Clock::time_point t0, spk_amg_info &info)
{
    const int L = r.levels();
    double tot = 0.0;
    for (int l = 0;; ++l) {
        info.rows[l] = r.rows(l);
        info.nnz[l] = r.nnz(l);
        tot += (double)info.nnz[l];
        if (l + 1 == L) break;
        double lmin = 0.0, lmax = 0.0, lo = 0.0, hi = 0.0;
        r.ritz(l, &lmin, &lmax);
        info.lambda_max[l] = lmax;
        smoother_interval(o, l, lmin, lmax, &lo, &hi);
        r.set_interval(l, lo, hi);
        r.regalerkin(l);
    }
    r.check();
    r.set_coarse_inverse(coarse_inverse(r.coarsest(), r.a_scale));
    info.operator_complexity = tot / (double)std::max<int64_t>(info.nnz[0], 1);
    info.setup_seconds = seconds_since(t0);
}

}  // namespace spk
