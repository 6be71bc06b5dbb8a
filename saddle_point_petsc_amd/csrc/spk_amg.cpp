// spk_amg.cpp -- smoothed-aggregation algebraic multigrid (-pc_type gamg): the hierarchy, built at KSPSetUp from the
// A00 block by one loop (build_levels) over two routes -- HostRoute: on the host, then uploaded (the default); DevRoute:
// on the device (-spk_gamg_setup device, kernels: spk_k_amg_setup.hip) -- and the cycle's launch sequence (kernels:
// spk_k_amg.hip): amg_apply walks the step list of spk_host.cpp's amg_cycle_steps (V or W), a tail run of coarse levels
// as one launch where the options ask for it (amg_plan_cycle).
// The same loop builds the grid-coarsened hierarchy (-pc_type mg, SPK_AMG_COARSEN_GRID): where the node grid is known a
// level halves its odd sides (-spk_mg_sides any: the even ones too) and P is the tensor product of linear interpolations -- no graph, no aggregation, no
// prolongator smoothing; everything else (Ritz values, Galerkin products, coarse inverse, refresh) is shared.
// -spk_mg_galerkin stencil (SPK_AMG_GALERKIN_STENCIL) forms the coarse operators of such a hierarchy by a gather on the
// node grid instead (spk_galerkin_core.hpp): both routes call it in coarsen_grid and, on new values, in regalerkin.
// -spk_mg_operator stencil (SPK_AMG_OPERATOR_STENCIL) has the cycle apply the levels between level 0 and the coarsest from
// their value arrays alone (spk_stencil_op_core.hpp): smooth(), the DOWN step and the tail descriptor dispatch on the
// level's flag, which amg_plan_cycle sets; the hierarchy is untouched.
// With reuse on (spk_pc_set_amg_reuse) a second, shorter loop (refresh_levels) over the same two routes puts new values
// of A00 through a hierarchy whose aggregates, prolongators and patterns stay.
//
// Every step is deterministic (fixed traversal orders, no hashing of pointers, a fixed Lanczos start vector): two
// builds of the same matrix give the same bytes, and so do two V-cycles.  DESIGN.md "Algebraic multigrid" has the
// algorithm and where it departs from PETSc's GAMG.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "spk_amg.hpp"
#include "spk_galerkin_core.hpp"
#include "spk_internal.hpp"

namespace spk {
void set_create_error(const std::string &m);   // spk_api.cpp: what spk_last_error(NULL) returns

namespace {

// columns sorted within each row (the caller's order is arbitrary); perm: where every sorted entry stood
void sort_rows(HostCsr &A, std::vector<int32_t> *perm = nullptr)
{
    struct Entry { int32_t first; double second; int32_t from; };
    std::vector<Entry> row;
    if (perm) perm->resize(A.ci.size());
    for (int32_t i = 0; i < A.nrows; ++i) {
        const int32_t k0 = A.rp[(size_t)i], k1 = A.rp[(size_t)i + 1];
        row.clear();
        for (int32_t k = k0; k < k1; ++k) row.push_back({A.ci[(size_t)k], A.v[(size_t)k], k});
        std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (int32_t k = k0; k < k1; ++k) {
            A.ci[(size_t)k] = row[(size_t)(k - k0)].first;
            A.v[(size_t)k] = row[(size_t)(k - k0)].second;
            if (perm) (*perm)[(size_t)k] = row[(size_t)(k - k0)].from;
        }
    }
}

// bs = 3 or 2 when the rows of every block row share one column list made of whole blocks, else 1
int detect_bs(const HostCsr &A)
{
    for (int bs : {3, 2}) {
        if (A.nrows % bs) continue;
        bool ok = true;
        for (int32_t r0 = 0; ok && r0 < A.nrows; r0 += bs) {
            const int32_t b0 = A.rp[(size_t)r0], len = A.rp[(size_t)r0 + 1] - b0;
            if (len % bs) { ok = false; break; }
            for (int k = 1; ok && k < bs; ++k) {
                const int32_t bk = A.rp[(size_t)r0 + k];
                if (A.rp[(size_t)r0 + k + 1] - bk != len) { ok = false; break; }
                for (int32_t j = 0; j < len; ++j)
                    if (A.ci[(size_t)(bk + j)] != A.ci[(size_t)(b0 + j)]) { ok = false; break; }
            }
            for (int32_t j = 0; ok && j < len; j += bs) {
                const int32_t c0 = A.ci[(size_t)(b0 + j)];
                if (c0 % bs) { ok = false; break; }
                for (int k = 1; k < bs; ++k)
                    if (A.ci[(size_t)(b0 + j + k)] != c0 + k) { ok = false; break; }
            }
        }
        if (ok) return bs;
    }
    return 1;
}

HostCsr transpose(const HostCsr &A)
{
    HostCsr T;
    T.nrows = A.ncols;
    T.ncols = A.nrows;
    T.rp.assign((size_t)T.nrows + 1, 0);
    for (int32_t c : A.ci) ++T.rp[(size_t)c + 1];
    for (int32_t i = 0; i < T.nrows; ++i) T.rp[(size_t)i + 1] += T.rp[(size_t)i];
    T.ci.resize(A.ci.size());
    T.v.resize(A.v.size());
    std::vector<int32_t> pos(T.rp.begin(), T.rp.end() - 1);
    for (int32_t i = 0; i < A.nrows; ++i)   // rows in order: the columns of T come out sorted
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) {
            const int32_t p = pos[(size_t)A.ci[(size_t)k]]++;
            T.ci[(size_t)p] = i;
            T.v[(size_t)p] = A.v[(size_t)k];
        }
    return T;
}

// C = A B (Gustavson, dense row accumulator; the sums run in A's then B's stored order; no entry is dropped)
HostCsr spgemm(const HostCsr &A, const HostCsr &B)
{
    HostCsr C;
    C.nrows = A.nrows;
    C.ncols = B.ncols;
    C.rp.assign((size_t)C.nrows + 1, 0);
    std::vector<double> acc((size_t)B.ncols, 0.0);
    std::vector<int32_t> mark((size_t)B.ncols, -1), cols;
    for (int32_t i = 0; i < A.nrows; ++i) {
        cols.clear();
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) {
            const int32_t r = A.ci[(size_t)k];
            const double a = A.v[(size_t)k];
            for (int32_t q = B.rp[(size_t)r]; q < B.rp[(size_t)r + 1]; ++q) {
                const int32_t j = B.ci[(size_t)q];
                if (mark[(size_t)j] != i) {
                    mark[(size_t)j] = i;
                    acc[(size_t)j] = 0.0;
                    cols.push_back(j);
                }
                acc[(size_t)j] += a * B.v[(size_t)q];
            }
        }
        std::sort(cols.begin(), cols.end());
        for (int32_t j : cols) {
            C.ci.push_back(j);
            C.v.push_back(acc[(size_t)j]);
        }
        C.rp[(size_t)i + 1] = (int32_t)C.ci.size();
    }
    return C;
}

// C = a A + b B over the union of the patterns (both sorted)
HostCsr add(double a, const HostCsr &A, double b, const HostCsr &B)
{
    HostCsr C;
    C.nrows = A.nrows;
    C.ncols = A.ncols;
    C.rp.assign((size_t)C.nrows + 1, 0);
    for (int32_t i = 0; i < A.nrows; ++i) {
        int32_t p = A.rp[(size_t)i], pe = A.rp[(size_t)i + 1], q = B.rp[(size_t)i], qe = B.rp[(size_t)i + 1];
        while (p < pe || q < qe) {
            const int32_t ca = p < pe ? A.ci[(size_t)p] : INT32_MAX, cb = q < qe ? B.ci[(size_t)q] : INT32_MAX;
            if (ca == cb) { C.ci.push_back(ca); C.v.push_back(a * A.v[(size_t)p++] + b * B.v[(size_t)q++]); }
            else if (ca < cb) { C.ci.push_back(ca); C.v.push_back(a * A.v[(size_t)p++]); }
            else { C.ci.push_back(cb); C.v.push_back(b * B.v[(size_t)q++]); }
        }
        C.rp[(size_t)i + 1] = (int32_t)C.ci.size();
    }
    return C;
}

std::vector<double> diag_inv(const HostCsr &A)
{
    std::vector<double> d((size_t)A.nrows);
    for (int32_t i = 0; i < A.nrows; ++i) {
        double a = 0.0;
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k)
            if (A.ci[(size_t)k] == i) a = A.v[(size_t)k];
        d[(size_t)i] = a == 0.0 ? 1.0 : 1.0 / a;   // as the device's PCJACOBI set-up
    }
    return d;
}

// number of eigenvalues of the symmetric tridiagonal (al, be[1..k)) below x (Sturm sequence)
int sturm_count(const std::vector<double> &al, const std::vector<double> &be, double x)
{
    int cnt = 0;
    double d = 1.0;
    for (size_t i = 0; i < al.size(); ++i) {
        const double b2 = i ? be[i] * be[i] : 0.0;
        d = al[i] - x - (i ? b2 / d : 0.0);
        if (d == 0.0) d = -1e-300;
        if (d < 0.0) ++cnt;
    }
    return cnt;
}

// extreme eigenvalues of the Lanczos tridiagonal (al, be[1..k)) by Sturm bisection: lmax from below, lmin from above
void ritz_extremes(const std::vector<double> &al, const std::vector<double> &be, double *lmin, double *lmax)
{
    double glo = al[0], ghi = al[0];   // Gershgorin bounds of the tridiagonal
    for (size_t i = 0; i < al.size(); ++i) {
        const double r = (i ? std::fabs(be[i]) : 0.0) + (i + 1 < al.size() ? std::fabs(be[i + 1]) : 0.0);
        glo = std::min(glo, al[i] - r);
        ghi = std::max(ghi, al[i] + r);
    }
    const int m = (int)al.size();
    double lo = glo, hi = ghi;
    for (int it = 0; it < 200 && hi - lo > 1e-15 * std::max(1.0, std::fabs(hi)); ++it) {
        const double mid = 0.5 * (lo + hi);
        if (sturm_count(al, be, mid) >= m) hi = mid; else lo = mid;
    }
    *lmax = lo;   // below the largest Ritz value
    lo = glo, hi = ghi;
    for (int it = 0; it < 200 && hi - lo > 1e-15 * std::max(1.0, std::fabs(hi)); ++it) {
        const double mid = 0.5 * (lo + hi);
        if (sturm_count(al, be, mid) >= 1) hi = mid; else lo = mid;
    }
    *lmin = hi;
}

constexpr int kLanczosSteps = 30;
static_assert(kLanczosSteps == lanczos_core::kSteps, "the state block of the resident route holds kLanczosSteps steps");

// extreme Ritz values of D^-1 A after kLanczosSteps Lanczos steps on the similar D^-1/2 A D^-1/2, from a fixed start vector.
// Ritz values lie inside the spectrum: both estimates approach from within (lmax from below).
// a_scale: a power of two; the steps run on a_scale A (every product with it is exact, and 1 changes no bit).  The refresh
// passes the one that brings A back to the binade it was built in, so that an operator rescaled by a power of two --
// where sqrt(d / 2) is no power-of-two multiple of sqrt(d) -- gives the Ritz values of the build to the bit.
void lanczos(const HostCsr &A, const std::vector<double> &dinv, double *lmin, double *lmax, double a_scale = 1.0)
{
    const int32_t n = A.nrows;
    std::vector<double> s((size_t)n), q((size_t)n), qp((size_t)n, 0.0), w((size_t)n), t((size_t)n);
    for (int32_t i = 0; i < n; ++i) s[(size_t)i] = std::sqrt(std::fabs(dinv[(size_t)i] / a_scale));
    double nq = 0.0;
    for (int32_t i = 0; i < n; ++i) {   // integer hash: the same start vector on every machine
        uint32_t h = (uint32_t)i * 2654435761u + 0x9e3779b9u;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        q[(size_t)i] = 0.5 + (double)(h & 0xffffu) / 65536.0;
        nq += q[(size_t)i] * q[(size_t)i];
    }
    nq = std::sqrt(nq);
    for (double &x : q) x /= nq;
    std::vector<double> al, be{0.0};
    const int k = (int)std::min<int64_t>(kLanczosSteps, n);
    for (int j = 0; j < k; ++j) {
        for (int32_t i = 0; i < n; ++i) t[(size_t)i] = s[(size_t)i] * q[(size_t)i];
        double a = 0.0;
        for (int32_t i = 0; i < n; ++i) {
            double acc = 0.0;
            for (int32_t p = A.rp[(size_t)i]; p < A.rp[(size_t)i + 1]; ++p) acc += A.v[(size_t)p] * t[(size_t)A.ci[(size_t)p]];
            w[(size_t)i] = s[(size_t)i] * (acc * a_scale);
            a += w[(size_t)i] * q[(size_t)i];
        }
        al.push_back(a);
        double nb = 0.0;
        for (int32_t i = 0; i < n; ++i) {
            w[(size_t)i] -= a * q[(size_t)i] + be.back() * qp[(size_t)i];
            nb += w[(size_t)i] * w[(size_t)i];
        }
        nb = std::sqrt(nb);
        if (j + 1 == k || nb <= 1e-12 * std::fabs(a)) break;
        be.push_back(nb);
        qp.swap(q);
        for (int32_t i = 0; i < n; ++i) q[(size_t)i] = w[(size_t)i] / nb;
    }
    ritz_extremes(al, be, lmin, lmax);
}

// strong-connection graph of the bs x bs nodes (sorted neighbour lists, the node itself left out)
void node_graph(const HostCsr &A, int bs, double theta, std::vector<int32_t> &gp, std::vector<int32_t> &gi)
{
    const int32_t nn = A.nrows / bs;
    std::vector<double> dn((size_t)nn, 0.0), acc((size_t)nn, 0.0);
    std::vector<int32_t> mark((size_t)nn, -1), cols;
    for (int32_t i = 0; i < A.nrows; ++i)
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k)
            if (A.ci[(size_t)k] / bs == i / bs) dn[(size_t)(i / bs)] += A.v[(size_t)k] * A.v[(size_t)k];
    for (double &d : dn) d = std::sqrt(d);
    gp.assign((size_t)nn + 1, 0);
    gi.clear();
    for (int32_t I = 0; I < nn; ++I) {
        cols.clear();
        for (int32_t r = I * bs; r < (I + 1) * bs; ++r)
            for (int32_t k = A.rp[(size_t)r]; k < A.rp[(size_t)r + 1]; ++k) {
                const int32_t J = A.ci[(size_t)k] / bs;
                if (J == I) continue;
                if (mark[(size_t)J] != I) { mark[(size_t)J] = I; acc[(size_t)J] = 0.0; cols.push_back(J); }
                acc[(size_t)J] += A.v[(size_t)k] * A.v[(size_t)k];
            }
        std::sort(cols.begin(), cols.end());
        for (int32_t J : cols)
            if (std::sqrt(acc[(size_t)J]) > theta * std::sqrt(dn[(size_t)I] * dn[(size_t)J])) gi.push_back(J);
        gp[(size_t)I + 1] = (int32_t)gi.size();
    }
}

// Vanek's greedy three-phase aggregation in node order; returns the number of aggregates
int32_t aggregate(const std::vector<int32_t> &gp, const std::vector<int32_t> &gi, std::vector<int32_t> &agg)
{
    const int32_t nn = (int32_t)gp.size() - 1;
    agg.assign((size_t)nn, -1);
    auto iso = [&](int32_t i) { return gp[(size_t)i] == gp[(size_t)i + 1]; };
    int32_t na = 0;
    // phase 1: a node whose strong neighbours are all free forms an aggregate with them
    for (int32_t i = 0; i < nn; ++i) {
        if (agg[(size_t)i] >= 0 || iso(i)) continue;
        bool free = true;
        for (int32_t k = gp[(size_t)i]; k < gp[(size_t)i + 1] && free; ++k) free = agg[(size_t)gi[(size_t)k]] < 0;
        if (!free) continue;
        agg[(size_t)i] = na;
        for (int32_t k = gp[(size_t)i]; k < gp[(size_t)i + 1]; ++k) agg[(size_t)gi[(size_t)k]] = na;
        ++na;
    }
    // phase 2: the rest join the phase-1 aggregate they have the most strong connections to (ties: lowest index)
    const std::vector<int32_t> a1 = agg;
    std::vector<std::pair<int32_t, int32_t>> cnt;
    for (int32_t i = 0; i < nn; ++i) {
        if (a1[(size_t)i] >= 0 || iso(i)) continue;
        cnt.clear();
        for (int32_t k = gp[(size_t)i]; k < gp[(size_t)i + 1]; ++k) {
            const int32_t a = a1[(size_t)gi[(size_t)k]];
            if (a < 0) continue;
            auto it = std::find_if(cnt.begin(), cnt.end(), [a](const auto &p) { return p.first == a; });
            if (it == cnt.end()) cnt.emplace_back(a, 1); else ++it->second;
        }
        int32_t best = -1, bc = 0;
        for (const auto &p : cnt)
            if (p.second > bc || (p.second == bc && p.first < best)) { best = p.first; bc = p.second; }
        agg[(size_t)i] = best;
    }
    // phase 3: the leftovers form aggregates with their free neighbours
    for (int32_t i = 0; i < nn; ++i) {
        if (agg[(size_t)i] >= 0 || iso(i)) continue;
        agg[(size_t)i] = na;
        for (int32_t k = gp[(size_t)i]; k < gp[(size_t)i + 1]; ++k)
            if (agg[(size_t)gi[(size_t)k]] < 0) agg[(size_t)gi[(size_t)k]] = na;
        ++na;
    }
    return na;
}

// bs columns per aggregate (the bs constant vectors), entries 1/sqrt(|aggregate|); isolated nodes: zero rows
HostCsr tentative(const std::vector<int32_t> &agg, int32_t na, int bs)
{
    std::vector<int32_t> size((size_t)na, 0);
    for (int32_t a : agg) if (a >= 0) ++size[(size_t)a];
    HostCsr P;
    P.nrows = (int32_t)agg.size() * bs;
    P.ncols = na * bs;
    P.rp.assign((size_t)P.nrows + 1, 0);
    for (size_t i = 0; i < agg.size(); ++i)
        for (int c = 0; c < bs; ++c) {
            const int32_t a = agg[i];
            if (a >= 0) {
                P.ci.push_back(a * bs + c);
                P.v.push_back(1.0 / std::sqrt((double)size[(size_t)a]));
            }
            P.rp[i * bs + c + 1] = (int32_t)P.ci.size();
        }
    return P;
}

// ---- grid coarsening (SPK_AMG_COARSEN_GRID): the halving rule and the tensor-product prolongator -------------------
// a direction of m nodes halves iff m is odd and >= 5 (SPK_AMG_SIDES_ODD), or m >= 4 (SPK_AMG_SIDES_ANY)
bool grid_halves(int32_t m, int sides) { return sides == SPK_AMG_SIDES_ANY ? m >= 4 : m >= 5 && (m & 1); }
// the coarse grid of `fd`; false when no direction halves.  A halved side of m nodes keeps m / 2 + 1: (m + 1) / 2 of an odd
// m; of an even m the fine indices 0, 2, ..., m - 2 and m - 1
bool grid_coarse_dims(const int32_t fd[3], int32_t cd[3], int sides)
{
    bool any = false;
    for (int a = 0; a < 3; ++a) {
        cd[a] = grid_halves(fd[a], sides) ? fd[a] / 2 + 1 : fd[a];
        any = any || cd[a] != fd[a];
    }
    return any;
}
// the parents of fine index i in one direction of m nodes: `first`, and one more behind it when cnt == 2 (weight 1/2 each,
// else 1).  An odd i that is the last index (m even) is a coarse node itself: the one parent m / 2
struct GridParents { int32_t first, cnt; };
GridParents grid_parents(int32_t i, int32_t m, bool halved)
{
    if (!halved) return {i, 1};
    if ((i & 1) && i == m - 1) return {(i + 1) / 2, 1};
    return (i & 1) ? GridParents{(i - 1) / 2, 2} : GridParents{i / 2, 1};
}
// entries of P = P_z (x) P_y (x) P_x (x) I_bs: per direction i + i/2 parents lie before fine index i; the last index of an
// even side has one parent, not two
int64_t grid_prolong_nnz(const int32_t fd[3], const int32_t cd[3], int bs)
{
    int64_t t = bs;
    for (int a = 0; a < 3; ++a) t *= cd[a] != fd[a] ? (int64_t)fd[a] + fd[a] / 2 - !(fd[a] & 1) : (int64_t)fd[a];
    return t;
}
// P as CSR with ascending columns, boundary nodes included: no special case for Dirichlet rows
HostCsr grid_prolongator(const int32_t fd[3], const int32_t cd[3], int bs)
{
    HostCsr P;
    P.nrows = fd[0] * fd[1] * fd[2] * bs;
    P.ncols = cd[0] * cd[1] * cd[2] * bs;
    P.rp.assign(1, 0);
    P.rp.reserve((size_t)P.nrows + 1);
    const size_t nz = (size_t)grid_prolong_nnz(fd, cd, bs);
    P.ci.reserve(nz);
    P.v.reserve(nz);
    for (int32_t k = 0; k < fd[2]; ++k)
        for (int32_t j = 0; j < fd[1]; ++j)
            for (int32_t i = 0; i < fd[0]; ++i) {
                const GridParents px = grid_parents(i, fd[0], cd[0] != fd[0]), py = grid_parents(j, fd[1], cd[1] != fd[1]),
                                  pz = grid_parents(k, fd[2], cd[2] != fd[2]);
                const double w = 1.0 / (double)(px.cnt * py.cnt * pz.cnt);   // 1, 1/2, 1/4 or 1/8
                for (int c = 0; c < bs; ++c) {
                    for (int32_t kk = 0; kk < pz.cnt; ++kk)
                        for (int32_t jj = 0; jj < py.cnt; ++jj)
                            for (int32_t ii = 0; ii < px.cnt; ++ii) {
                                P.ci.push_back((((pz.first + kk) * cd[1] + py.first + jj) * cd[0] + px.first + ii) * bs + c);
                                P.v.push_back(w);
                            }
                    P.rp.push_back((int32_t)P.ci.size());
                }
            }
    return P;
}

// dense inverse of the SPD coarsest operator through Cholesky (symmetrised); a_scale as in lanczos: the factor is that
// of a_scale A and the inverse is scaled back, both exactly
std::vector<double> coarse_inverse(const HostCsr &A, double a_scale = 1.0)
{
    const int32_t n = A.nrows;
    std::vector<double> L((size_t)n * n, 0.0), X((size_t)n * n, 0.0);
    for (int32_t i = 0; i < n; ++i)
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) L[(size_t)i * n + A.ci[(size_t)k]] = A.v[(size_t)k] * a_scale;
    for (int32_t j = 0; j < n; ++j) {
        double d = L[(size_t)j * n + j];
        for (int32_t k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0.0)) fail(SPK_ERR_ARG, "amg: the coarsest operator (%d equations) is not positive definite", (int)n);
        d = std::sqrt(d);
        L[(size_t)j * n + j] = d;
        for (int32_t i = j + 1; i < n; ++i) {
            double s = L[(size_t)i * n + j];
            for (int32_t k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = s / d;
        }
    }
    std::vector<double> y((size_t)n);
    for (int32_t c = 0; c < n; ++c) {   // L L^T x = e_c
        for (int32_t i = 0; i < n; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int32_t k = 0; k < i; ++k) s -= L[(size_t)i * n + k] * y[(size_t)k];
            y[(size_t)i] = s / L[(size_t)i * n + i];
        }
        for (int32_t i = n - 1; i >= 0; --i) {
            double s = y[(size_t)i];
            for (int32_t k = i + 1; k < n; ++k) s -= L[(size_t)k * n + i] * X[(size_t)k * n + c];
            X[(size_t)i * n + c] = s / L[(size_t)i * n + i];
        }
    }
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = i + 1; j < n; ++j) {
            const double s = 0.5 * (X[(size_t)i * n + j] + X[(size_t)j * n + i]);
            X[(size_t)i * n + j] = X[(size_t)j * n + i] = s;
        }
    if (a_scale != 1.0)
        for (double &x : X) x *= a_scale;
    return X;
}

using Clock = std::chrono::steady_clock;
double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// sum |D_0^-1|: exactly homogeneous under a power of two (every partial sum scales with it), so its binade tells by
// which power of two an operator was rescaled since the build
double abs_sum(const std::vector<double> &x)
{
    double t = 0.0;
    for (double v : x) t += std::fabs(v);
    return t;
}
// the power of two that brings an operator with this sum |D^-1| back to the binade of the one with sum `built`
double binade_scale(double built, double now)
{
    if (!(built > 0.0) || !(now > 0.0) || !std::isfinite(built) || !std::isfinite(now)) return 1.0;
    return std::ldexp(1.0, std::ilogb(now) - std::ilogb(built));   // A grew by 2^k: |D^-1| shrank by it, A is scaled by 2^-k
}

// the smoother's interval on level l from the extreme Ritz values: the esteig rule and its refusal, for both loops
void smoother_interval(const spk_amg_opts &o, int l, double lmin, double lmax, double *lo, double *hi)
{
    *lo = o.esteig[0] * lmin + o.esteig[1] * lmax, *hi = o.esteig[2] * lmin + o.esteig[3] * lmax;
    if (o.smoother == SPK_AMG_CHEBYSHEV && !(*lo > 0.0 && *hi > *lo))
        fail(SPK_ERR_ARG, "amg: Chebyshev interval [%g, %g] on level %d is empty or not positive (esteig)", *lo, *hi, l);
}

// what the application's options make of the levels `info` lists: after every build and every refresh, on both routes
// (build_levels clears the info and the host-route refresh copies the host's over it)
void fill_cycle_info(const spk_amg_opts &o, spk_amg_info &info)
{
    info.cycle = o.cycle;
    info.op = o.op;
    info.tail_first = amg_tail_first(info.levels, info.rows, o.cycle, o.tail, o.tail_rows);
    info.tail_launches = info.tail_first < 0 ? 0 : (int32_t)amg_tail_runs(amg_cycle_steps(info.levels, o.cycle), info.tail_first).size();
}

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
        if (grid) {   // the grid is known: no graph, no aggregation, no prolongator smoothing
            if (!grid_coarse_dims(fd, cd, o.sides)) { stuck = true; break; }
            double lmin = 0.0, lmax = 0.0, lo = 0.0, hi = 0.0;
            r.ritz(l, &lmin, &lmax);
            info.lambda_max[l] = lmax;
            smoother_interval(o, l, lmin, lmax, &lo, &hi);
            r.set_interval(l, lo, hi);
            r.coarsen_grid(l, bs, fd, cd);
            std::memcpy(fd, cd, sizeof fd);
            continue;
        }
        std::vector<int32_t> gp, gi, agg;
        r.graph(l, bs, o.threshold, gp, gi);
        const int32_t na = aggregate(gp, gi, agg);
        if (na == 0 || (int64_t)na * bs >= n) break;   // no coarsening left
        double lmin = 0.0, lmax = 0.0;
        r.ritz(l, &lmin, &lmax);
        info.lambda_max[l] = lmax;
        double lo = 0.0, hi = 0.0;
        smoother_interval(o, l, lmin, lmax, &lo, &hi);
        r.set_interval(l, lo, hi);
        r.coarsen(l, bs, std::move(agg), na, 4.0 / (3.0 * lmax), o.nsmooths);
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

// the host route: every matrix a HostCsr of h.lv (level 0 and its D^-1 are there before the loop runs)
struct HostRoute {
    AmgHier &h;
    double a_scale = 1.0;   // the refresh's (see lanczos)
    AmgLevel &lv(int l) const { return h.lv[(size_t)l]; }
    int32_t rows(int l) const { return lv(l).A.nrows; }
    int64_t nnz(int l) const { return lv(l).A.nnz(); }
    void graph(int l, int bs, double theta, std::vector<int32_t> &gp, std::vector<int32_t> &gi) const { node_graph(lv(l).A, bs, theta, gp, gi); }
    void ritz(int l, double *lmin, double *lmax) const { lanczos(lv(l).A, lv(l).dinv, lmin, lmax, a_scale); }
    void set_interval(int l, double lo, double hi) const { lv(l).lo = lo, lv(l).hi = hi; }
    void coarsen(int l, int bs, std::vector<int32_t> agg, int32_t na, double omega, int nsmooths) const
    {
        AmgLevel &L = lv(l);
        L.agg = std::move(agg);
        L.Ptent = tentative(L.agg, na, bs);
        L.P = L.Ptent;
        for (int s = 0; s < nsmooths; ++s) {   // P = (I - omega D^-1 A) P
            HostCsr AP = spgemm(L.A, L.P);
            for (int32_t i = 0; i < AP.nrows; ++i)
                for (int32_t k = AP.rp[(size_t)i]; k < AP.rp[(size_t)i + 1]; ++k) AP.v[(size_t)k] *= L.dinv[(size_t)i];
            L.P = add(1.0, L.P, -omega, AP);
        }
        galerkin(l);
    }
    void coarsen_grid(int l, int bs, const int32_t fd[3], const int32_t cd[3]) const
    {
        if (grid_prolong_nnz(fd, cd, bs) > INT32_MAX)
            fail(SPK_ERR_UNSUPPORTED, "amg: the prolongator of level %d has more entries than 32-bit offsets address", l);
        lv(l).P = grid_prolongator(fd, cd, bs);
        if (h.o.galerkin != SPK_AMG_GALERKIN_STENCIL) return galerkin(l);
        if (galerkin::gs_nnz(cd, bs) > INT32_MAX)
            fail(SPK_ERR_UNSUPPORTED, "amg: the operator of level %d has more entries than 32-bit offsets address", l + 1);
        if (l == 0) galerkin_stencil_check_host(fd, bs, lv(0).A.rp.data(), lv(0).A.ci.data());
        lv(l).R = transpose(lv(l).P);
        h.lv.emplace_back();
        HostCsr &N = h.lv.back().A;
        N.nrows = N.ncols = cd[0] * cd[1] * cd[2] * bs;
        N.rp.assign((size_t)N.nrows + 1, 0);
        N.ci.assign((size_t)galerkin::gs_nnz(cd, bs), 0);
        N.v.assign(N.ci.size(), 0.0);
        stencil(l, fd, cd, bs);
    }
    // level l+1 by the grid-stencil gather (SPK_AMG_GALERKIN_STENCIL), the build's and the refresh's: pattern, values, D^-1
    void stencil(int l, const int32_t fd[3], const int32_t cd[3], int bs) const
    {
        const HostCsr &F = lv(l).A;
        HostCsr &N = lv(l + 1).A;
        galerkin_stencil_host(fd, cd, bs, F.rp.data(), F.ci.data(), F.v.data(), N.rp.data(), N.ci.data(), N.v.data());
        lv(l + 1).dinv = diag_inv(N);
    }
    // R = P^T and level l+1 from the P of level l
    void galerkin(int l) const
    {
        AmgLevel &L = lv(l);
        L.R = transpose(L.P);
        HostCsr Ac = spgemm(L.R, spgemm(L.A, L.P));
        h.lv.emplace_back();   // (L dangles from here)
        h.lv.back().A = add(0.5, Ac, 0.5, transpose(Ac));   // exactly symmetric (the products agree to rounding)
        h.lv.back().dinv = diag_inv(h.lv.back().A);
    }
    int levels() const { return (int)h.lv.size(); }
    void regalerkin(int l) const
    {
        if (h.info.galerkin == SPK_AMG_GALERKIN_STENCIL) return stencil(l, h.info.dims[l], h.info.dims[l + 1], h.info.block_size);
        AmgLevel &L = lv(l), &N = lv(l + 1);
        const HostCsr Ac = spgemm(L.R, spgemm(L.A, L.P));
        HostCsr An = add(0.5, Ac, 0.5, transpose(Ac));
        if (An.rp != N.A.rp || An.ci != N.A.ci)   // (no product drops an entry: the patterns follow from the kept ones)
            fail(SPK_ERR_STATE, "amg: the refreshed operator of level %d has another pattern than the kept one", l + 1);
        N.A.v = std::move(An.v);
        N.dinv = diag_inv(N.A);
    }
    void check() const {}
    const HostCsr &coarsest() const { return h.lv.back().A; }
    void set_coarse_inverse(std::vector<double> cinv) const { h.cinv = std::move(cinv); }
};

// the test hooks' copy-out, shared by the host hierarchy and the download of a device-built one
void csr_out(const HostCsr &M, const CsrOut &o)
{
    o.sizes(M.nrows, M.ncols, M.nnz());
    if (o.rowptr) std::memcpy(o.rowptr, M.rp.data(), sizeof(int32_t) * M.rp.size());
    if (o.colidx && M.nnz()) std::memcpy(o.colidx, M.ci.data(), sizeof(int32_t) * M.ci.size());
    if (o.val && M.nnz()) std::memcpy(o.val, M.v.data(), sizeof(double) * M.v.size());
}

// SPK_AMG_COARSE_INV: the dense n x n inverse as full CSR rows
void coarse_inv_out(int32_t n, const double *cinv, const CsrOut &o)
{
    o.sizes(n, n, (int64_t)n * n);
    for (int32_t i = 0; o.rowptr && i <= n; ++i) o.rowptr[i] = i * n;
    for (int64_t k = 0; o.colidx && k < (int64_t)n * n; ++k) o.colidx[k] = (int32_t)(k % n);
    if (o.val) std::memcpy(o.val, cinv, sizeof(double) * (size_t)n * n);
}

// what a query for matrix `which` of level l refuses on a hierarchy of L levels
void check_level_query(int L, int l, int which)
{
    if (l < 0 || l >= L) fail(SPK_ERR_ARG, "amg: level %d outside [0,%d)", l, L);
    if (which == SPK_AMG_COARSE_INV && l != L - 1) fail(SPK_ERR_ARG, "amg: the coarse inverse lives on level %d", L - 1);
    if (which < SPK_AMG_OP || which > SPK_AMG_COARSE_INV) fail(SPK_ERR_ARG, "amg: unknown matrix %d", which);
    if ((which == SPK_AMG_PROLONG || which == SPK_AMG_TENTATIVE) && l == L - 1) fail(SPK_ERR_ARG, "amg: the coarsest level has no prolongator");
}

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

}  // namespace

void amg_check_opts(const spk_amg_opts &o, bool host_builder)
{
    if (o.max_levels < 1 || o.max_levels > SPK_AMG_MAX_LEVELS)
        fail(SPK_ERR_ARG, "amg: max_levels %d outside [1,%d]", o.max_levels, SPK_AMG_MAX_LEVELS);
    if (o.coarse_eq_limit < 1) fail(SPK_ERR_ARG, "amg: coarse_eq_limit %d < 1", o.coarse_eq_limit);
    if (o.nsmooths < 0 || o.nsmooths > 4) fail(SPK_ERR_ARG, "amg: nsmooths %d outside [0,4]", o.nsmooths);
    if (o.smoother != SPK_AMG_CHEBYSHEV && o.smoother != SPK_AMG_RICHARDSON) fail(SPK_ERR_ARG, "amg: unknown smoother %d", o.smoother);
    if (!(o.threshold >= 0.0) || !std::isfinite(o.threshold)) fail(SPK_ERR_ARG, "amg: threshold must be >= 0");
    if (o.smooth_its < 1 || o.smooth_its > 64) fail(SPK_ERR_ARG, "amg: smooth_its %d outside [1,64]", o.smooth_its);
    if (o.block_size < 0 || o.block_size > 3) fail(SPK_ERR_ARG, "amg: block_size %d outside [0,3]", o.block_size);
    for (double e : o.esteig)
        if (!std::isfinite(e)) fail(SPK_ERR_ARG, "amg: esteig factors must be finite");
    if (!(o.richardson_scale > 0.0) || !std::isfinite(o.richardson_scale)) fail(SPK_ERR_ARG, "amg: richardson_scale must be > 0");
    if (o.setup != SPK_AMG_SETUP_HOST && o.setup != SPK_AMG_SETUP_DEVICE)
        fail(SPK_ERR_ARG, "amg: setup %d is neither SPK_AMG_SETUP_HOST (0) nor SPK_AMG_SETUP_DEVICE (1)", o.setup);
    if (o.coarsening != SPK_AMG_COARSEN_AGGREGATION && o.coarsening != SPK_AMG_COARSEN_GRID)
        fail(SPK_ERR_ARG, "amg: coarsening %d is neither SPK_AMG_COARSEN_AGGREGATION (0) nor SPK_AMG_COARSEN_GRID (1)", o.coarsening);
    if (o.coarsening == SPK_AMG_COARSEN_GRID) {   // (grid, transfer, sides and galerkin are read under grid coarsening only)
        if (o.grid[0] < 2 || o.grid[1] < 2 || o.grid[2] < 1)
            fail(SPK_ERR_ARG, "amg: grid %d x %d x %d: at least 2 x 2 nodes (x 1 in 2-D)", o.grid[0], o.grid[1], o.grid[2]);
        if ((int64_t)o.grid[0] * o.grid[1] > INT32_MAX || (int64_t)o.grid[0] * o.grid[1] * o.grid[2] > INT32_MAX)
            fail(SPK_ERR_ARG, "amg: grid %d x %d x %d has more nodes than 32-bit rows address", o.grid[0], o.grid[1], o.grid[2]);
        if (o.transfer != SPK_AMG_TRANSFER_MATRIX_FREE && o.transfer != SPK_AMG_TRANSFER_STORED)
            fail(SPK_ERR_ARG, "amg: transfer %d is neither SPK_AMG_TRANSFER_MATRIX_FREE (0) nor SPK_AMG_TRANSFER_STORED (1)", o.transfer);
        if (o.sides != SPK_AMG_SIDES_ODD && o.sides != SPK_AMG_SIDES_ANY)
            fail(SPK_ERR_ARG, "amg: sides %d is neither SPK_AMG_SIDES_ODD (0) nor SPK_AMG_SIDES_ANY (1)", o.sides);
        if (o.galerkin != SPK_AMG_GALERKIN_PRODUCTS && o.galerkin != SPK_AMG_GALERKIN_STENCIL)
            fail(SPK_ERR_ARG, "amg: galerkin %d is neither SPK_AMG_GALERKIN_PRODUCTS (0) nor SPK_AMG_GALERKIN_STENCIL (1)", o.galerkin);
        if (o.transfer == SPK_AMG_TRANSFER_MATRIX_FREE && (o.grid[1] > 65535 || o.grid[2] > 65535))   // they are launch dimensions
            fail(SPK_ERR_UNSUPPORTED, "amg: the matrix-free transfers take at most 65535 nodes in y and z (grid %d x %d x %d) -- "
                 "use -spk_mg_transfer stored", o.grid[0], o.grid[1], o.grid[2]);
    }
    if (o.cycle != SPK_AMG_CYCLE_V && o.cycle != SPK_AMG_CYCLE_W)
        fail(SPK_ERR_ARG, "amg: cycle %d is neither SPK_AMG_CYCLE_V (0) nor SPK_AMG_CYCLE_W (1)", o.cycle);
    if (o.tail != SPK_AMG_TAIL_AUTO && o.tail != SPK_AMG_TAIL_LAUNCHES && o.tail != SPK_AMG_TAIL_FUSED)
        fail(SPK_ERR_ARG, "amg: tail %d is none of SPK_AMG_TAIL_AUTO (0), SPK_AMG_TAIL_LAUNCHES (1), SPK_AMG_TAIL_FUSED (2)", o.tail);
    if (o.tail_rows < 0) fail(SPK_ERR_ARG, "amg: tail_rows %d < 0 (0: the default of %d)", o.tail_rows, SPK_AMG_TAIL_ROWS_DEFAULT);
    if (o.op != SPK_AMG_OPERATOR_CSR && o.op != SPK_AMG_OPERATOR_STENCIL)
        fail(SPK_ERR_ARG, "amg: op %d is neither SPK_AMG_OPERATOR_CSR (0) nor SPK_AMG_OPERATOR_STENCIL (1)", o.op);
    if (o.op == SPK_AMG_OPERATOR_STENCIL && o.coarsening != SPK_AMG_COARSEN_GRID)
        fail(SPK_ERR_UNSUPPORTED, "amg: -spk_mg_operator stencil applies levels whose pattern is the grid stencil's closed form; "
             "smoothed aggregation (gamg) has none -- use -pc_type mg with -spk_mg_galerkin stencil, or -spk_mg_operator csr");
    if (o.op == SPK_AMG_OPERATOR_STENCIL && o.galerkin != SPK_AMG_GALERKIN_STENCIL)
        fail(SPK_ERR_UNSUPPORTED, "amg: -spk_mg_operator stencil applies levels whose pattern is the grid stencil's closed form; "
             "only -spk_mg_galerkin stencil guarantees it (the generic products keep whatever pattern they meet) -- pass "
             "-spk_mg_galerkin stencil, or -spk_mg_operator csr");
    if (o.lanczos != SPK_AMG_LANCZOS_STEPWISE && o.lanczos != SPK_AMG_LANCZOS_RESIDENT)
        fail(SPK_ERR_ARG, "amg: lanczos %d is neither SPK_AMG_LANCZOS_STEPWISE (0) nor SPK_AMG_LANCZOS_RESIDENT (1)", o.lanczos);
    if (!host_builder && o.lanczos == SPK_AMG_LANCZOS_RESIDENT && o.setup == SPK_AMG_SETUP_HOST)
        fail(SPK_ERR_UNSUPPORTED, "amg: -spk_amg_lanczos resident keeps the scalars of the device set-up's Lanczos on the device; the "
             "host set-up has no device Lanczos -- pass -spk_gamg_setup device, or -spk_amg_lanczos stepwise");
}

void amg_build(AmgHier &h, HostCsr A, const spk_amg_opts &o)
{
    const auto t0 = Clock::now();
    amg_check_opts(o, true);   // (the host builder reads neither setup nor lanczos: it range-checks both)
    if (A.nrows != A.ncols || A.nrows <= 0) fail(SPK_ERR_ARG, "amg: the operator must be square and non-empty");
    std::vector<int32_t> perm;
    sort_rows(A, &perm);
    h = AmgHier{};
    h.o = o;
    h.perm = std::move(perm);
    h.lv.emplace_back();
    h.lv[0].A = std::move(A);
    h.lv[0].dinv = diag_inv(h.lv[0].A);
    h.dinv_sum = abs_sum(h.lv[0].dinv);
    HostRoute r{h};
    build_levels(r, o.block_size > 0 ? o.block_size : detect_bs(h.lv[0].A), o, SPK_AMG_SETUP_HOST, t0, h.info);
    fill_cycle_info(o, h.info);
}

void amg_refresh(AmgHier &h, const double *val)
{
    const auto t0 = Clock::now();
    if (h.lv.empty()) fail(SPK_ERR_STATE, "amg: no hierarchy to refresh (an earlier refresh failed)");
    AmgLevel &F = h.lv[0];
    for (size_t k = 0; k < F.A.v.size(); ++k) F.A.v[k] = val[(size_t)h.perm[k]];
    F.dinv = diag_inv(F.A);
    HostRoute r{h, binade_scale(h.dinv_sum, abs_sum(F.dinv))};
    try {
        refresh_levels(r, h.o, t0, h.info);
        fill_cycle_info(h.o, h.info);
    } catch (...) {   // half-refreshed: never to be read or applied
        h.lv.clear();
        h.cinv.clear();
        std::memset(&h.info, 0, sizeof h.info);
        throw;
    }
}

void AmgHier::level(int l, int which, const CsrOut &out) const
{
    check_level_query((int)lv.size(), l, which);
    const AmgLevel &V = lv[(size_t)l];
    if (which == SPK_AMG_COARSE_INV) coarse_inv_out(V.A.nrows, cinv.data(), out);
    else csr_out(which == SPK_AMG_OP ? V.A : which == SPK_AMG_PROLONG || o.coarsening == SPK_AMG_COARSEN_GRID ? V.P : V.Ptent, out);
}

}  // namespace spk

// ---------------------------------------------------------------------------
// the context's hierarchy: built from its A00 (single rank: the diagonal block is all of A), uploaded, applied
// ---------------------------------------------------------------------------
namespace spk {

// the node size the options ask for, else the blocking the context found for its A layout (0: detect from the pattern)
static int ctx_block_size(const spk_ctx *c, const spk_amg_opts &o)
{
    if (o.block_size > 0) return o.block_size;
    if (c->Adict.ok) return c->Adict.bs;
    return c->spmv_format == 1 ? 2 : c->spmv_format == 2 ? 3 : 0;
}

static HostCsr dev_csr_download(const CsrDev &A, bool values, hipStream_t s)
{
    HostCsr H;
    H.nrows = A.nrows;
    H.ncols = A.ncols;
    H.rp.resize((size_t)A.nrows + 1);
    SPK_HIP(hipMemcpyAsync(H.rp.data(), A.rowptr.p, sizeof(int32_t) * H.rp.size(), hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    H.ci.resize((size_t)H.rp[(size_t)A.nrows]);
    H.v.resize(H.ci.size());
    if (!H.ci.empty()) {
        SPK_HIP(hipMemcpyAsync(H.ci.data(), A.colidx.p, sizeof(int32_t) * H.ci.size(), hipMemcpyDeviceToHost, s));
        if (values) SPK_HIP(hipMemcpyAsync(H.v.data(), A.val.p, sizeof(double) * H.v.size(), hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
    }
    return H;
}

std::unique_ptr<spk_amg_hier> amg_build_ctx(spk_ctx *c)
{
    spk_amg_opts o = c->amg_opts;
    o.block_size = ctx_block_size(c, o);
    auto h = std::make_unique<spk_amg_hier>();
    amg_build(h->h, dev_csr_download(c->Ad, true, c->stream), o);
    return h;
}

static void upload_host_csr(CsrDev &D, const HostCsr &H)
{
    D.nrows = H.nrows;
    D.ncols = H.ncols;
    D.nnz = H.nnz();
    D.rowptr.upload(H.rp.data(), H.rp.size());
    D.colidx.upload(H.ci.data(), H.ci.size(), 4);
    D.val.upload(H.v.data(), H.v.size(), 4);
}

// the smoothing steps of a level from its interval [lo, hi]
static void smoother_coeffs(AmgLevelDev &D, const spk_amg_opts &o, double lo, double hi)
{
    const int nu = o.smooth_its;
    D.alpha.assign((size_t)nu, o.richardson_scale);
    D.beta.assign((size_t)nu, 0.0);
    if (o.smoother == SPK_AMG_CHEBYSHEV) {   // Saad, Alg. 12.1: d_k = rho_k rho_{k-1} d_{k-1} + 2 rho_k / delta D^-1 r_k
        const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
        double rho = 1.0 / sigma;
        D.alpha[0] = 1.0 / theta;
        for (int k = 1; k < nu; ++k) {
            const double rn = 1.0 / (2.0 * sigma - rho);
            D.alpha[(size_t)k] = 2.0 * rn / delta;
            D.beta[(size_t)k] = rn * rho;
            rho = rn;
        }
    }
}

// the V-cycle's vectors; level 0 takes the context's padded length, as the layouts' products want them.  Both callers
// pass c->ld, the device build even before pc_setup's own ensure_vectors: every set_block ends in ensure_vectors and
// nothing else changes n_local or m, so c->ld is current whenever the context holds an operator (pc_setup asks for one).
static void alloc_cycle_vectors(AmgDev &d, int64_t ld)
{
    const size_t L = d.lv.size();
    for (size_t l = 0; l < L; ++l) {
        AmgLevelDev &D = d.lv[l];
        const size_t nv = l == 0 ? (size_t)ld : (size_t)D.n;
        if (l > 0) D.b.alloc(nv, 8);
        D.ya.alloc(nv, 16);
        D.yb.alloc(nv, 16);
        if (l == 0 && L > 1) D.t.alloc(nv, 16);
    }
}

// The application's plan, rebuilt at every set-up (build or refresh) from the options and the levels as they are now:
// the steps of the cycle, the tail runs, and -- where there is a tail -- the kernel's descriptor and step list on the
// device: the pointers, the smoothing coefficients and, per step, the buffer that holds the iterate (smooth()'s rule:
// every smoothing step writes the buffer its input is not in; PRE0 starts into ya; the coarse solve writes ya).
static void amg_plan_cycle(AmgDev &d, const spk_amg_opts &o)
{
    fill_cycle_info(o, d.info);
    const int L = (int)d.lv.size(), t = d.info.tail_first, nu = o.smooth_its;
    // (amg_check_opts: the option comes with grid coarsening and the stencil products, so these levels have the closed form)
    for (int l = 0; l < L; ++l) d.lv[(size_t)l].stencil_op = o.op == SPK_AMG_OPERATOR_STENCIL && l >= 1 && l + 1 < L;
    d.steps = amg_cycle_steps(L, o.cycle);
    d.runs = amg_tail_runs(d.steps, t);
    d.run_sel.assign(d.runs.size(), 0);
    d.tsteps.clear();
    d.tail_stencil = false;
    if (t < 0) {
        d.tail_desc.release();
        d.tail_steps.release();
        return;
    }
    if (d.steps.size() > (size_t)INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "amg: the cycle has more steps than 32 bits count");
    d.tsteps.resize(d.steps.size());
    int32_t sel[SPK_AMG_MAX_LEVELS] = {};
    size_t run = 0;
    for (size_t i = 0; i < d.steps.size(); ++i) {
        const AmgStep st = d.steps[i];
        d.tsteps[i] = k::AmgTailStep{st.kind, st.level, sel[st.level], st.level + 1 < L ? sel[st.level + 1] : 0};
        if (st.kind == SPK_AMG_STEP_PRE0) sel[st.level] = (nu & 1) ? 0 : 1;
        else if (st.kind == SPK_AMG_STEP_PRE || st.kind == SPK_AMG_STEP_POST) sel[st.level] ^= nu & 1;
        else if (st.kind == SPK_AMG_STEP_COARSE) sel[st.level] = 0;
        if (run < d.runs.size() && (size_t)d.runs[run].second == i + 1) d.run_sel[run++] = sel[t];   // where the run leaves level t's iterate
    }
    auto desc = std::make_unique<k::AmgTailDesc>();
    std::memset(desc.get(), 0, sizeof *desc);
    d.tail_steps.upload(d.tsteps.data(), d.tsteps.size());
    desc->cinv = d.cinv.p;
    desc->steps = d.tail_steps.p;
    desc->first = t;
    desc->levels = L;
    for (int l = t; l < L; ++l) {
        AmgLevelDev &D = d.lv[(size_t)l];
        k::AmgTailLevel &V = desc->lv[l];
        V.arp = D.A.rowptr.p, V.aci = D.A.colidx.p, V.av = D.A.val.p;
        V.dinv = D.dinv.p;
        V.b = D.b.p, V.ya = D.ya.p, V.yb = D.yb.p;
        V.n = D.n;
        V.nu = nu;
        if (l + 1 == L) continue;
        V.nc = d.lv[(size_t)l + 1].n;
        V.prp = D.P.rowptr.p, V.pci = D.P.colidx.p, V.pv = D.P.val.p;
        V.rrp = D.R.rowptr.p, V.rci = D.R.colidx.p, V.rv = D.R.val.p;
        V.matrix_free = D.grid.matrix_free ? 1 : 0;
        V.stencil = D.stencil_op ? 1 : 0;
        d.tail_stencil = d.tail_stencil || D.stencil_op;
        if (D.grid.on) std::memcpy(V.nd, D.grid.fd, sizeof V.nd);
        if (D.grid.on) V.g = k::grid_args(D.grid), V.bs = D.grid.bs, V.fz = D.grid.fd[2];
        for (int q = 0; q < nu; ++q) V.alpha[q] = D.alpha[(size_t)q], V.beta[q] = D.beta[(size_t)q];
    }
    d.tail_desc.upload(desc.get(), 1);
}

// reuse on: what the next set-up compares before it refreshes -- the options, the sizes and a device copy of the
// diagonal block's pattern as the context stores it
static void keep_pattern(spk_ctx *c, AmgDev &d)
{
    if (!d.reuse) d.reuse = std::make_unique<AmgReuse>();
    AmgReuse &ru = *d.reuse;
    ru.o = c->amg_opts;
    ru.bs = ctx_block_size(c, c->amg_opts);
    ru.n = c->n_local;
    ru.nnz = c->Ad.nnz;
    ru.ld = c->ld;
    ru.rowptr.alloc_raw((size_t)ru.n + 1);
    ru.colidx.alloc_raw((size_t)ru.nnz);
    ru.flag.alloc(2);
    SPK_HIP(hipMemcpyAsync(ru.rowptr.p, c->Ad.rowptr.p, sizeof(int32_t) * ((size_t)ru.n + 1), hipMemcpyDeviceToDevice, c->stream));
    if (ru.nnz)
        SPK_HIP(hipMemcpyAsync(ru.colidx.p, c->Ad.colidx.p, sizeof(int32_t) * (size_t)ru.nnz, hipMemcpyDeviceToDevice, c->stream));
}

void amg_upload(spk_ctx *c, std::unique_ptr<spk_amg_hier> hp)
{
    const auto t0 = Clock::now();
    const AmgHier &h = hp->h;
    auto d = std::make_unique<AmgDev>();
    const size_t L = h.lv.size();
    std::vector<AmgLevelDev>(L).swap(d->lv);   // (the levels own device buffers: constructed in place, never moved)
    for (size_t l = 0; l < L; ++l) {
        const AmgLevel &H = h.lv[l];
        AmgLevelDev &D = d->lv[l];
        D.n = H.A.nrows;
        if (l > 0) {
            upload_host_csr(D.A, H.A);
            D.dinv.upload(H.dinv.data(), H.dinv.size(), 8);
        }
        if (l + 1 == L) break;
        upload_host_csr(D.P, H.P);
        upload_host_csr(D.R, H.R);
        smoother_coeffs(D, h.o, H.lo, H.hi);
        if (h.info.coarsening == SPK_AMG_COARSEN_GRID) D.grid.set(h.info.dims[l], h.info.dims[l + 1], h.info.block_size, h.o.transfer);
    }
    d->cinv.upload(h.cinv.data(), h.cinv.size());
    alloc_cycle_vectors(*d, c->ld);
    if (c->amg_reuse) keep_pattern(c, *d);
    SPK_HIP(hipDeviceSynchronize());
    d->info = h.info;
    amg_plan_cycle(*d, h.o);
    d->info.setup_seconds += seconds_since(t0);
    c->amg_d = std::move(d);
    c->amg_h = std::move(hp);
}

// ---------------------------------------------------------------------------
// the device route (-spk_gamg_setup device; kernels: spk_k_amg_setup.hip).  Per level: node graph -> host (the greedy
// aggregation is sequential by definition and runs unchanged, so the aggregates and every pattern are the host
// route's) -> tentative prolongator, Lanczos, the products and transposes as kernels.  Only the graph, the aggregates,
// the Lanczos scalars and the coarsest operator cross the bus.
// ---------------------------------------------------------------------------
namespace {

int32_t scan_counts(const int32_t *cnt, int32_t n, int32_t *out, hipStream_t s)   // out[0..n]; returns out[n]
{
    DevBuf<int32_t> scr;
    scr.alloc_raw((size_t)n / 2048 + 8);
    k::exclusive_scan_i32(cnt, n, out, scr.p, s);
    int32_t tot = 0;
    SPK_HIP(hipMemcpyAsync(&tot, out + n, sizeof tot, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    return tot;
}

void dev_csr_values(CsrDev &C, int64_t nnz)
{
    C.nnz = nnz;
    C.colidx.alloc_raw((size_t)nnz, 4);
    C.val.alloc_raw((size_t)nnz, 4);
}

void dev_csr_copy(CsrDev &C, const CsrDev &A, hipStream_t s)
{
    C.nrows = A.nrows;
    C.ncols = A.ncols;
    C.rowptr.alloc_raw((size_t)A.nrows + 1, 8);
    dev_csr_values(C, A.nnz);
    SPK_HIP(hipMemcpyAsync(C.rowptr.p, A.rowptr.p, sizeof(int32_t) * ((size_t)A.nrows + 1), hipMemcpyDeviceToDevice, s));
    if (A.nnz) {
        SPK_HIP(hipMemcpyAsync(C.colidx.p, A.colidx.p, sizeof(int32_t) * (size_t)A.nnz, hipMemcpyDeviceToDevice, s));
        SPK_HIP(hipMemcpyAsync(C.val.p, A.val.p, sizeof(double) * (size_t)A.nnz, hipMemcpyDeviceToDevice, s));
    }
}

// C = A B (sorted columns, no entry dropped, each entry summed in A's stored order, then B's)
void dev_spgemm(CsrDev &C, const CsrDev &A, const CsrDev &B, hipStream_t s)
{
    const int32_t n = A.nrows;
    C.nrows = n;
    C.ncols = B.ncols;
    DevBuf<int32_t> bound, off, cnt, sc;
    DevBuf<double> sv;
    DevBuf<unsigned long long> tot;
    bound.alloc_raw((size_t)n, 8);
    off.alloc_raw((size_t)n + 1, 8);
    cnt.alloc_raw((size_t)n, 8);
    tot.alloc(1);
    k::amgs_spgemm_bound(A, B, bound.p, tot.p, s);
    unsigned long long slots = 0;
    SPK_HIP(hipMemcpyAsync(&slots, tot.p, sizeof slots, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    if (slots > (unsigned long long)INT32_MAX)
        fail(SPK_ERR_UNSUPPORTED, "amg: a sparse product of the device set-up needs %llu scratch slots, more than its 32-bit "
             "offsets address -- use -spk_gamg_setup host", slots);
    scan_counts(bound.p, n, off.p, s);
    sc.alloc_raw((size_t)slots, 4);
    sv.alloc_raw((size_t)slots, 4);
    k::amgs_spgemm_expand(A, B, off.p, sc.p, sv.p, cnt.p, s);
    C.rowptr.alloc_raw((size_t)n + 1, 8);
    dev_csr_values(C, scan_counts(cnt.p, n, C.rowptr.p, s));
    k::amgs_compact(n, off.p, C.rowptr.p, sc.p, sv.p, C.colidx.p, C.val.p, s);
    SPK_HIP(hipStreamSynchronize(s));   // the scratch goes out of scope
}

// C = a A + b diag(scale) B over the union pattern
void dev_add(CsrDev &C, double a, const CsrDev &A, double b, const CsrDev &B, const double *scale, hipStream_t s)
{
    const int32_t n = A.nrows;
    C.nrows = n;
    C.ncols = A.ncols;
    DevBuf<int32_t> cnt;
    cnt.alloc_raw((size_t)n, 8);
    k::amgs_add(a, A, b, B, scale, nullptr, nullptr, nullptr, cnt.p, s);
    C.rowptr.alloc_raw((size_t)n + 1, 8);
    dev_csr_values(C, scan_counts(cnt.p, n, C.rowptr.p, s));
    k::amgs_add(a, A, b, B, scale, C.rowptr.p, C.colidx.p, C.val.p, nullptr, s);
    SPK_HIP(hipStreamSynchronize(s));
}

void dev_transpose(CsrDev &T, const CsrDev &A, hipStream_t s)
{
    T.nrows = A.ncols;
    T.ncols = A.nrows;
    DevBuf<int32_t> cnt, pos;
    cnt.alloc_raw((size_t)T.nrows, 8);
    pos.alloc_raw((size_t)T.nrows, 8);
    SPK_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * (size_t)T.nrows, s));
    k::amgs_col_count(A.colidx.p, A.nnz, cnt.p, s);
    T.rowptr.alloc_raw((size_t)T.nrows + 1, 8);
    dev_csr_values(T, scan_counts(cnt.p, T.nrows, T.rowptr.p, s));
    SPK_HIP(hipMemcpyAsync(pos.p, T.rowptr.p, sizeof(int32_t) * (size_t)T.nrows, hipMemcpyDeviceToDevice, s));
    k::amgs_transpose_fill(A, pos.p, T.colidx.p, T.val.p, s);
    k::amgs_sort_rows(T.rowptr.p, T.colidx.p, T.val.p, T.nrows, s);
    SPK_HIP(hipStreamSynchronize(s));
}

// the 30 Lanczos steps of `lanczos` with the level's own product (level 0: the context's layout, else the CSR kernel);
// the two sums of a step come back to the host, which keeps the tridiagonal and the break rule
// tri (the test hook's): the tridiagonal itself;  *reads += the read-backs made
struct LzTri { std::vector<double> al, be; };
void dev_lanczos(spk_ctx *c, const CsrDev *A, int32_t n, int64_t nv, const double *dinv, double *lmin, double *lmax,
                 double a_scale = 1.0, int32_t *reads = nullptr, LzTri *tri = nullptr)
{
    hipStream_t s = c->stream;
    DevBuf<double> sv, q, qp, w, t, aw, res;
    for (DevBuf<double> *b : {&sv, &q, &qp, &w, &t, &aw}) b->alloc((size_t)nv, 16);
    res.alloc(8);
    const k::Finish f = c->fin(res.p);
    auto sum = [&]() {
        double h = 0.0;
        SPK_HIP(hipMemcpyAsync(&h, res.p, sizeof h, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        if (reads) ++*reads;
        return h;
    };
    k::amgs_lz_init(n, dinv, 1.0 / a_scale, sv.p, q.p, f, s);
    const double nq = std::sqrt(sum());
    k::amgs_lz_scale(n, nq, q.p, sv.p, q.p, t.p, s);
    std::vector<double> al, be{0.0};
    const int kk = (int)std::min<int64_t>(kLanczosSteps, n);
    double *qc = q.p, *qo = qp.p;
    for (int j = 0; j < kk; ++j) {
        if (A) k::amg_spmv(*A, t.p, aw.p, nullptr, s);
        else a_mult(c, t.p, aw.p, nullptr, nullptr, nullptr, false, nullptr);
        k::amgs_lz_dot(n, sv.p, aw.p, a_scale, w.p, qc, f, s);
        const double a = sum();
        al.push_back(a);
        k::amgs_lz_update(n, a, be.back(), qc, qo, w.p, f, s);
        const double nb = std::sqrt(sum());
        if (j + 1 == kk || nb <= 1e-12 * std::fabs(a)) break;
        be.push_back(nb);
        std::swap(qc, qo);
        k::amgs_lz_scale(n, nb, w.p, sv.p, qc, t.p, s);
    }
    c->check_device_error();
    if (tri) tri->al = al, tri->be = be;
    ritz_extremes(al, be, lmin, lmax);
}

// What the resident route (SPK_AMG_LANCZOS_RESIDENT) owns for a whole build or refresh: the six vectors, sized once for
// level 0's padded length, and the state block.  No level allocates; a level clears what it uses (dev_lanczos gets its
// vectors zeroed too: the first update reads qp, and level 0's product reads t over the padded length).
struct LzWork {
    DevBuf<double> v;
    DevBuf<lanczos_core::LzState> st;
    size_t cap = 0;   // doubles per vector
    static size_t stride(int64_t nv) { return ((size_t)nv + 16 + 31) / 32 * 32; }   // 256-byte aligned, like an allocation of its own
    void ensure(int64_t nv)
    {
        if (v.p && stride(nv) <= cap) return;
        cap = stride(nv);
        v.alloc_raw(6 * cap);
        st.alloc_raw(1);
    }
};

// dev_lanczos without the host in the loop: all kk steps enqueued blind, the scalars in the state block (the rule:
// spk_lanczos_core.hpp), the kernels behind the break returning at their entry (the product still runs, on a stale t into
// aw, which nothing reads); one read of the block per call.  The sums are dev_lanczos's to the bit, so is the tridiagonal.
void dev_lanczos_resident(spk_ctx *c, LzWork &wk, const CsrDev *A, int32_t n, int64_t nv, const double *dinv, double *lmin,
                          double *lmax, double a_scale = 1.0, int32_t *reads = nullptr, LzTri *tri = nullptr)
{
    hipStream_t s = c->stream;
    wk.ensure(nv);
    const size_t ld = LzWork::stride(nv);
    double *sv = wk.v.p, *q = sv + ld, *qp = q + ld, *w = qp + ld, *t = w + ld, *aw = t + ld;
    lanczos_core::LzState *st = wk.st.p;
    SPK_HIP(hipMemsetAsync(wk.v.p, 0, sizeof(double) * 6 * ld, s));
    SPK_HIP(hipMemsetAsync(st, 0, sizeof *st, s));
    const k::Finish f = c->fin(nullptr);
    k::amgs_lz_init_resident(n, dinv, 1.0 / a_scale, sv, q, f, st, s);
    k::amgs_lz_scale_resident(n, -1, q, sv, q, t, st, s);
    const int kk = (int)std::min<int64_t>(kLanczosSteps, n);
    double *qc = q, *qo = qp;
    for (int j = 0; j < kk; ++j) {
        if (A) k::amg_spmv(*A, t, aw, nullptr, s);
        else a_mult(c, t, aw, nullptr, nullptr, nullptr, false, nullptr);
        k::amgs_lz_dot_resident(n, j, sv, aw, a_scale, w, qc, f, st, s);
        k::amgs_lz_update_resident(n, j, kk, qc, qo, w, f, st, s);
        if (j + 1 == kk) break;
        std::swap(qc, qo);
        k::amgs_lz_scale_resident(n, j + 1, w, sv, qc, t, st, s);
    }
    lanczos_core::LzState h;
    SPK_HIP(hipMemcpyAsync(&h, st, sizeof h, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    if (reads) ++*reads;
    c->check_device_error();
    if (h.steps < 1 || h.steps > kk) fail(SPK_ERR_HIP, "amg: the resident Lanczos reports %d steps of %d", (int)h.steps, kk);
    const std::vector<double> al(h.al, h.al + h.steps), be(h.be, h.be + h.steps);
    if (tri) tri->al = al, tri->be = be;
    ritz_extremes(al, be, lmin, lmax);
}

// sum |x| in the fixed order of the sentinel finish (abs_sum of the host: exactly homogeneous under a power of two)
double dev_abs_sum(spk_ctx *c, const double *x, int32_t n, DevBuf<double> &res)
{
    hipStream_t s = c->stream;
    k::amgs_abs_sum(n, x, c->fin(res.p), s);
    double h = 0.0;
    SPK_HIP(hipMemcpyAsync(&h, res.p, sizeof h, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    c->check_device_error();
    return h;
}

// the context's CSR as it is when every row ascends, else a sorted copy in `copy`
const CsrDev &sorted_rows(spk_ctx *c, CsrDev &copy)
{
    hipStream_t s = c->stream;
    DevBuf<int32_t> flag;
    flag.alloc(1);
    k::amgs_rows_sorted(c->Ad.rowptr.p, c->Ad.colidx.p, c->n_local, flag.p, s);
    int32_t unsorted = 0;
    SPK_HIP(hipMemcpyAsync(&unsorted, flag.p, sizeof unsorted, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    if (!unsorted) return c->Ad;
    dev_csr_copy(copy, c->Ad, s);
    k::amgs_sort_rows(copy.rowptr.p, copy.colidx.p, copy.val.p, c->n_local, s);
    return copy;
}

// the device route: every matrix a CsrDev of d.lv.  Level 0 is special, throughout and only here: its operator is A0 (the
// context's CSR or the sorted copy), its D^-1 is dinv0 (pc_setup computes the context's afterwards), its Lanczos product
// the context's layout over vectors of the padded length; with one level it is the coarsest too.
struct DevRoute {
    spk_ctx *c;
    AmgDev &d;
    const spk_amg_opts &o;
    const CsrDev &A0;
    const double *dinv0;
    hipStream_t s;
    bool keep = false;        // reuse on: coarsen keeps A_l P_l and R_l A_l P_l for regalerkin
    int32_t *err = nullptr;   // regalerkin's error word
    double a_scale = 1.0;     // the refresh's (see lanczos)
    mutable LzWork work;             // SPK_AMG_LANCZOS_RESIDENT: the vectors and the state block of every level's Lanczos
    mutable int32_t readbacks = 0;   // device -> host reads of the Ritz estimates (spk_amg_info.ritz_readbacks)
    // the route's part of the info, behind build_levels / refresh_levels
    void ritz_info(spk_amg_info &info) const { info.lanczos = o.lanczos, info.ritz_readbacks = readbacks; }
    const CsrDev &A(int l) const { return l == 0 ? A0 : d.lv[(size_t)l].A; }
    const double *dinv(int l) const { return l == 0 ? dinv0 : d.lv[(size_t)l].dinv.p; }
    int32_t rows(int l) const { return A(l).nrows; }
    int64_t nnz(int l) const { return A(l).nnz; }

    // norms of the diagonal blocks, count, scan, fill; then to the host
    void graph(int l, int bs, double theta, std::vector<int32_t> &gp, std::vector<int32_t> &gi) const
    {
        const CsrDev &M = A(l);
        const int32_t nn = M.nrows / bs;
        DevBuf<double> dn;
        DevBuf<int32_t> cnt, gpd, gid;
        dn.alloc_raw((size_t)nn, 8);
        cnt.alloc_raw((size_t)nn, 8);
        gpd.alloc_raw((size_t)nn + 1, 8);
        k::amgs_node_norms(M.rowptr.p, M.colidx.p, M.val.p, nn, bs, dn.p, s);
        k::amgs_graph(M.rowptr.p, M.colidx.p, M.val.p, nn, bs, theta, dn.p, nullptr, cnt.p, s);
        const int32_t ne = scan_counts(cnt.p, nn, gpd.p, s);
        gid.alloc_raw((size_t)ne, 8);
        k::amgs_graph(M.rowptr.p, M.colidx.p, M.val.p, nn, bs, theta, dn.p, gpd.p, gid.p, s);
        gp.resize((size_t)nn + 1);
        gi.resize((size_t)ne);
        SPK_HIP(hipMemcpyAsync(gp.data(), gpd.p, sizeof(int32_t) * gp.size(), hipMemcpyDeviceToHost, s));
        if (ne) SPK_HIP(hipMemcpyAsync(gi.data(), gid.p, sizeof(int32_t) * gi.size(), hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
    }
    // Under SPK_AMG_GALERKIN_STENCIL a level >= 1 holds the host route's bytes, so where it is small enough to cross the bus
    // as the coarsest operator does (at most SPK_AMG_MAX_COARSE rows) the host's own Lanczos runs on a download of it: the
    // host's Ritz values to the bit, and one download where the device steps read two sums back 30 times.  It is on such
    // levels that the bits matter: 30 steps without reorthogonalisation on a few dozen rows lose orthogonality altogether
    // before the largest Ritz value has converged, and its value then follows the rounding of every sum
    bool ritz_on_host(int l) const
    {
        return o.coarsening == SPK_AMG_COARSEN_GRID && o.galerkin == SPK_AMG_GALERKIN_STENCIL && l > 0 && rows(l) <= SPK_AMG_MAX_COARSE;
    }
    void ritz(int l, double *lmin, double *lmax) const
    {
        if (ritz_on_host(l)) {
            const HostCsr H = dev_csr_download(A(l), true, s);
            ++readbacks;
            return lanczos(H, diag_inv(H), lmin, lmax, a_scale);
        }
        const CsrDev *M = l ? &A(l) : nullptr;
        const int64_t nv = l ? rows(l) : c->ld;
        if (o.lanczos == SPK_AMG_LANCZOS_RESIDENT) dev_lanczos_resident(c, work, M, rows(l), nv, dinv(l), lmin, lmax, a_scale, &readbacks);
        else dev_lanczos(c, M, rows(l), nv, dinv(l), lmin, lmax, a_scale, &readbacks);
    }
    void set_interval(int l, double lo, double hi) { smoother_coeffs(d.lv[(size_t)l], o, lo, hi); }
    void coarsen(int l, int bs, std::vector<int32_t> agg, int32_t na, double omega, int nsmooths)
    {
        AmgLevelDev &L = d.lv[(size_t)l];
        const int32_t n = rows(l);
        {   // tentative prolongator: 1/sqrt(|aggregate|) comes from the host, like the aggregates
            std::vector<int32_t> size((size_t)na, 0);
            for (int32_t a : agg) if (a >= 0) ++size[(size_t)a];
            std::vector<double> inv((size_t)na);
            for (int32_t a = 0; a < na; ++a) inv[(size_t)a] = 1.0 / std::sqrt((double)size[(size_t)a]);
            DevBuf<int32_t> aggd, cnt;
            DevBuf<double> invd;
            aggd.upload(agg.data(), agg.size(), 8);
            invd.upload(inv.data(), inv.size(), 8);
            cnt.alloc_raw((size_t)n, 8);
            CsrDev &T = L.Ptent;
            T.nrows = n;
            T.ncols = na * bs;
            k::amgs_tent_count(aggd.p, n, bs, cnt.p, s);
            T.rowptr.alloc_raw((size_t)n + 1, 8);
            dev_csr_values(T, scan_counts(cnt.p, n, T.rowptr.p, s));
            k::amgs_tent_fill(aggd.p, invd.p, n, bs, T.rowptr.p, T.colidx.p, T.val.p, s);
            SPK_HIP(hipStreamSynchronize(s));
        }
        L.agg = std::move(agg);
        dev_csr_copy(L.P, L.Ptent, s);
        for (int it = 0; it < nsmooths; ++it) {   // P = (I - omega D^-1 A) P
            CsrDev AP, Pn;
            dev_spgemm(AP, A(l), L.P, s);
            dev_add(Pn, 1.0, L.P, -omega, AP, dinv(l), s);
            L.P = std::move(Pn);
        }
        galerkin(l);
    }
    // P from the node grids alone: every row length is known, so one kernel writes row pointers, columns and weights
    void coarsen_grid(int l, int bs, const int32_t fd[3], const int32_t cd[3])
    {
        AmgLevelDev &L = d.lv[(size_t)l];
        const int64_t nz = grid_prolong_nnz(fd, cd, bs);
        if (nz > INT32_MAX)
            fail(SPK_ERR_UNSUPPORTED, "amg: the prolongator of level %d has more entries than 32-bit offsets address", l);
        L.grid.set(fd, cd, bs, o.transfer);
        L.P.nrows = rows(l);
        L.P.ncols = cd[0] * cd[1] * cd[2] * bs;
        L.P.rowptr.alloc_raw((size_t)L.P.nrows + 1, 8);
        dev_csr_values(L.P, nz);
        k::amgs_grid_prolongator(L.grid, L.P.rowptr.p, L.P.colidx.p, L.P.val.p, s);
        if (o.galerkin != SPK_AMG_GALERKIN_STENCIL) return galerkin(l);
        const int64_t nc = galerkin::gs_nnz(cd, bs);
        if (nc > INT32_MAX)
            fail(SPK_ERR_UNSUPPORTED, "amg: the operator of level %d has more entries than 32-bit offsets address", l + 1);
        dev_transpose(L.R, L.P, s);
        d.lv.emplace_back();   // (reserved)
        AmgLevelDev &N = d.lv.back();
        N.n = N.A.nrows = N.A.ncols = L.P.ncols;
        N.A.rowptr.alloc_raw((size_t)N.n + 1, 8);
        dev_csr_values(N.A, nc);
        N.dinv.alloc((size_t)N.n, 8);
        DevBuf<unsigned long long> bad;   // (row << 32 | column) of the first entry outside the stencil, else all ones
        if (l == 0) {   // level 0 alone has a foreign pattern: its one check, read back behind the level's launches
            bad.alloc_raw(1);
            SPK_HIP(hipMemsetAsync(bad.p, 0xff, sizeof(unsigned long long), s));
            k::amgs_galerkin_stencil_check(L.grid, A(0), bad.p, s);
        }
        stencil(l);
        if (l == 0) {
            unsigned long long key = 0;
            SPK_HIP(hipMemcpyAsync(&key, bad.p, sizeof key, hipMemcpyDeviceToHost, s));
            SPK_HIP(hipStreamSynchronize(s));
            if (key != ~0ull)
                fail(SPK_ERR_UNSUPPORTED, "amg: the entry in row %d, column %d of the operator couples nodes that are not neighbours "
                     "on the %d x %d x %d grid; the stencil products take couplings between neighbouring nodes only -- use "
                     "-spk_mg_galerkin products", (int)(key >> 32), (int)(key & 0xffffffffull), (int)fd[0], (int)fd[1], (int)fd[2]);
        }
    }
    // level l+1 by the grid-stencil gather, the build's and the refresh's: three launches into buffers whose sizes follow
    // from the node grids -- no count, no scan, no scratch, no read-back
    void stencil(int l)
    {
        AmgLevelDev &L = d.lv[(size_t)l], &N = d.lv[(size_t)l + 1];
        k::amgs_galerkin_stencil(L.grid, A(l), N.A, s);
        k::extract_diag_inv(N.A, N.dinv.p, s);
    }
    // R = P^T and level l+1 from the P of level l
    void galerkin(int l)
    {
        AmgLevelDev &L = d.lv[(size_t)l];
        dev_transpose(L.R, L.P, s);
        CsrDev AP, Ac, AcT;
        dev_spgemm(AP, A(l), L.P, s);
        dev_spgemm(Ac, L.R, AP, s);
        dev_transpose(AcT, Ac, s);
        d.lv.emplace_back();   // (reserved)
        AmgLevelDev &N = d.lv.back();
        dev_add(N.A, 0.5, Ac, 0.5, AcT, nullptr, s);   // exactly symmetric (the products agree to rounding)
        N.n = N.A.nrows;
        N.dinv.alloc((size_t)N.n, 8);
        k::extract_diag_inv(N.A, N.dinv.p, s);
        if (keep) {
            AmgLevelDev &K = d.lv[(size_t)l];
            K.AP = std::move(AP);
            K.Ac = std::move(Ac);
        }
    }
    int levels() const { return (int)d.lv.size(); }
    // three launches into buffers the build left: nothing is allocated, counted or scanned
    void regalerkin(int l)
    {
        if (o.galerkin == SPK_AMG_GALERKIN_STENCIL) return stencil(l);
        AmgLevelDev &L = d.lv[(size_t)l], &N = d.lv[(size_t)l + 1];
        k::amgs_spgemm_numeric(A(l), L.P, L.AP, err, s);
        k::amgs_spgemm_numeric(L.R, L.AP, L.Ac, err, s);
        k::amgs_symmetrise_numeric(L.Ac, N.A, err, s);
        k::extract_diag_inv(N.A, N.dinv.p, s);
    }
    void check() const
    {
        int32_t bad = 0;
        SPK_HIP(hipMemcpyAsync(&bad, err, sizeof bad, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        if (bad) fail(SPK_ERR_STATE, "amg: a product of the refresh has no slot in the kept pattern");
    }
    HostCsr coarsest() const { return dev_csr_download(A((int)d.lv.size() - 1), true, s); }
    void set_coarse_inverse(const std::vector<double> &cinv) { d.cinv.upload(cinv.data(), cinv.size()); }
};

}  // namespace

std::unique_ptr<AmgDev> amg_build_device(spk_ctx *c)
{
    const auto t0 = Clock::now();
    const spk_amg_opts &o = c->amg_opts;
    amg_check_opts(o);
    c->ensure_scratch();
    if (c->n_local <= 0) fail(SPK_ERR_ARG, "amg: the operator must be square and non-empty");
    auto d = std::make_unique<AmgDev>();
    if (c->amg_reuse) d->reuse = std::make_unique<AmgReuse>();   // level 0's sorted copy and D^-1 outlive the build
    CsrDev copy_here;
    DevBuf<double> dinv0_here;
    CsrDev &copy = d->reuse ? d->reuse->sorted : copy_here;
    DevBuf<double> &dinv0 = d->reuse ? d->reuse->dinv0 : dinv0_here;
    const CsrDev &A0 = sorted_rows(c, copy);
    if (d->reuse) d->reuse->use_sorted = &A0 == &copy;
    const int cbs = ctx_block_size(c, o), bs = cbs > 0 ? cbs : detect_bs(dev_csr_download(A0, false, c->stream));
    d->lv.reserve((size_t)o.max_levels);   // the levels own device buffers and never move
    d->lv.emplace_back();
    d->lv[0].n = c->n_local;
    dinv0.alloc((size_t)c->n_local, 8);
    k::extract_diag_inv(c->Ad, dinv0.p, c->stream);
    if (d->reuse) {
        d->reuse->sum.alloc(8);
        d->reuse->dinv_sum = dev_abs_sum(c, dinv0.p, c->n_local, d->reuse->sum);
    }
    DevRoute r{c, *d, o, A0, dinv0.p, c->stream, d->reuse != nullptr, nullptr, 1.0, {}, 0};
    build_levels(r, bs, o, SPK_AMG_SETUP_DEVICE, t0, d->info);
    r.ritz_info(d->info);
    alloc_cycle_vectors(*d, c->ld);
    amg_plan_cycle(*d, o);
    if (d->reuse) keep_pattern(c, *d);
    SPK_HIP(hipDeviceSynchronize());
    d->info.setup_seconds = seconds_since(t0);   // the vectors count too, up to the synchronise
    return d;
}

bool amg_can_refresh(spk_ctx *c)
{
    if (!c->amg_reuse || !c->amg_on || !c->amg_d || !c->amg_d->reuse) return false;
    AmgReuse &ru = *c->amg_d->reuse;
    const spk_amg_opts &a = c->amg_opts, &b = ru.o;
    bool same = a.max_levels == b.max_levels && a.coarse_eq_limit == b.coarse_eq_limit && a.nsmooths == b.nsmooths &&
                a.smoother == b.smoother && a.threshold == b.threshold && a.smooth_its == b.smooth_its &&
                a.block_size == b.block_size && a.richardson_scale == b.richardson_scale && a.setup == b.setup &&
                a.coarsening == b.coarsening && a.transfer == b.transfer && a.sides == b.sides && a.galerkin == b.galerkin &&
                a.lanczos == b.lanczos;
    // (cycle, tail, tail_rows and op steer the application, not the hierarchy: not compared)
    for (int i = 0; i < 4; ++i) same = same && a.esteig[i] == b.esteig[i];
    for (int i = 0; i < 3; ++i) same = same && a.grid[i] == b.grid[i];
    if (!same || ctx_block_size(c, a) != ru.bs || c->n_local != ru.n || c->Ad.nnz != ru.nnz || c->ld != ru.ld) return false;
    if ((a.setup == SPK_AMG_SETUP_HOST) != (c->amg_h != nullptr)) return false;
    hipStream_t s = c->stream;
    SPK_HIP(hipMemsetAsync(ru.flag.p, 0, 2 * sizeof(int32_t), s));
    k::amgs_pattern_equal(ru.rowptr.p, c->Ad.rowptr.p, (int64_t)ru.n + 1, ru.flag.p, s);
    k::amgs_pattern_equal(ru.colidx.p, c->Ad.colidx.p, ru.nnz, ru.flag.p, s);
    int32_t differ = 1;
    SPK_HIP(hipMemcpyAsync(&differ, ru.flag.p, sizeof differ, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    return differ == 0;
}

void amg_refresh_ctx(spk_ctx *c)
{
    const auto t0 = Clock::now();
    hipStream_t s = c->stream;
    AmgDev &d = *c->amg_d;
    AmgReuse &ru = *d.reuse;
    const size_t L = d.lv.size();
    // cycle, tail, tail_rows and op steer the application, not the hierarchy (amg_can_refresh does not compare them): the
    // refresh takes the ones this set-up was given
    ru.o.cycle = c->amg_opts.cycle, ru.o.tail = c->amg_opts.tail, ru.o.tail_rows = c->amg_opts.tail_rows, ru.o.op = c->amg_opts.op;
    if (c->amg_h) {   // the host route: the values down, the host refresh, the values of the levels up
        AmgHier &h = c->amg_h->h;
        h.o.cycle = ru.o.cycle, h.o.tail = ru.o.tail, h.o.tail_rows = ru.o.tail_rows, h.o.op = ru.o.op;
        std::vector<double> val((size_t)c->Ad.nnz);
        if (!val.empty()) SPK_HIP(hipMemcpyAsync(val.data(), c->Ad.val.p, sizeof(double) * val.size(), hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        amg_refresh(h, val.data());
        for (size_t l = 0; l < L; ++l) {
            const AmgLevel &H = h.lv[l];
            AmgLevelDev &D = d.lv[l];
            if (l > 0) {
                if (H.A.nnz()) SPK_HIP(hipMemcpyAsync(D.A.val.p, H.A.v.data(), sizeof(double) * H.A.v.size(), hipMemcpyHostToDevice, s));
                SPK_HIP(hipMemcpyAsync(D.dinv.p, H.dinv.data(), sizeof(double) * H.dinv.size(), hipMemcpyHostToDevice, s));
            }
            if (l + 1 < L) smoother_coeffs(D, h.o, H.lo, H.hi);
        }
        SPK_HIP(hipMemcpyAsync(d.cinv.p, h.cinv.data(), sizeof(double) * h.cinv.size(), hipMemcpyHostToDevice, s));
        SPK_HIP(hipDeviceSynchronize());   // (the host vectors are pageable: the copies have left them by now anyway)
        d.info = h.info;
    } else {
        c->ensure_scratch();
        if (ru.use_sorted) {   // the build's sorted copy of level 0 again, in its buffers
            if (ru.nnz) {
                SPK_HIP(hipMemcpyAsync(ru.sorted.colidx.p, c->Ad.colidx.p, sizeof(int32_t) * (size_t)ru.nnz, hipMemcpyDeviceToDevice, s));
                SPK_HIP(hipMemcpyAsync(ru.sorted.val.p, c->Ad.val.p, sizeof(double) * (size_t)ru.nnz, hipMemcpyDeviceToDevice, s));
            }
            k::amgs_sort_rows(ru.sorted.rowptr.p, ru.sorted.colidx.p, ru.sorted.val.p, ru.n, s);
        }
        k::extract_diag_inv(c->Ad, ru.dinv0.p, s);
        const double a_scale = binade_scale(ru.dinv_sum, dev_abs_sum(c, ru.dinv0.p, ru.n, ru.sum));
        DevRoute r{c, d, ru.o, ru.use_sorted ? ru.sorted : c->Ad, ru.dinv0.p, s, true, ru.flag.p + 1, a_scale, {}, 0};
        refresh_levels(r, ru.o, t0, d.info);
        r.ritz_info(d.info);
        SPK_HIP(hipDeviceSynchronize());
    }
    amg_plan_cycle(d, ru.o);   // the coefficients are new, and the device route's coarse inverse lies elsewhere
    d.info.setup_seconds = seconds_since(t0);
}

void amg_drop_reuse(spk_ctx *c)
{
    if (!c->amg_d || !c->amg_d->reuse) return;
    c->amg_d->reuse.reset();
    for (AmgLevelDev &D : c->amg_d->lv) {
        D.AP = CsrDev{};
        D.Ac = CsrDev{};
    }
}

// the test hooks: the host hierarchy where pc_setup kept one, else one download from the device-built levels
void amg_ctx_level(spk_ctx *c, int l, int which, const CsrOut &out)
{
    if (c->amg_h) return c->amg_h->h.level(l, which, out);
    const AmgDev &d = *c->amg_d;
    check_level_query((int)d.lv.size(), l, which);
    const AmgLevelDev &V = d.lv[(size_t)l];
    if (which == SPK_AMG_COARSE_INV) {
        std::vector<double> cinv(out.val ? (size_t)V.n * V.n : 0);
        if (out.val) SPK_HIP(hipMemcpy(cinv.data(), d.cinv.p, sizeof(double) * cinv.size(), hipMemcpyDeviceToHost));
        return coarse_inv_out(V.n, cinv.data(), out);
    }
    const bool grid = d.info.coarsening == SPK_AMG_COARSEN_GRID;   // no tentative prolongator: SPK_AMG_TENTATIVE is P
    const CsrDev &M = which == SPK_AMG_OP ? (l == 0 ? c->Ad : V.A) : which == SPK_AMG_PROLONG || grid ? V.P : V.Ptent;
    if (!out.rowptr && !out.colidx && !out.val) return out.sizes(M.nrows, M.ncols, M.nnz);   // nothing to download
    HostCsr H = dev_csr_download(M, true, c->stream);
    if (which == SPK_AMG_OP && l == 0) sort_rows(H);   // the context's CSR keeps the caller's order
    csr_out(H, out);
}

void amg_ctx_aggregates(spk_ctx *c, int l, int32_t *nnodes, int32_t *agg)
{
    if (c->amg_h) aggregates_out(c->amg_h->h.lv, c->amg_d->info, l, nnodes, agg);
    else aggregates_out(c->amg_d->lv, c->amg_d->info, l, nnodes, agg);
}

// the test hook of the transfers: one launch on copies of the caller's vectors
void amg_debug_transfer(spk_ctx *c, int l, int which, int stored, int64_t fine_len, const double *a, const double *b, double *out)
{
    AmgDev &d = *c->amg_d;
    if (l < 0 || l + 1 >= (int)d.lv.size()) fail(SPK_ERR_ARG, "amg: level %d has no transfer", l);
    if ((which != 0 && which != 1) || (stored != 0 && stored != 1)) fail(SPK_ERR_ARG, "amg: transfer hook: which and stored are 0 or 1");
    AmgLevelDev &D = d.lv[(size_t)l];
    const int64_t nf = D.n, nc = d.lv[(size_t)l + 1].n;
    if (fine_len < nf) fail(SPK_ERR_ARG, "amg: transfer hook: %lld entries for the %lld rows of level %d", (long long)fine_len, (long long)nf, l);
    if (!stored && !D.grid.on) fail(SPK_ERR_STATE, "amg: level %d was not built by the grid rule: it has no matrix-free transfer", l);
    hipStream_t s = c->stream;
    DevBuf<double> da, db, dout;
    const int64_t na = which == 0 ? nc : fine_len, nb = fine_len, no = which == 0 ? fine_len : nc;
    da.upload(a, (size_t)na, 16);
    db.upload(b, (size_t)nb, 16);
    if (which == 0) {   // out = y + P e, in place on the copy of y
        if (stored) k::amg_prolong_add(D.P, da.p, db.p, nullptr, s);
        else k::amg_prolong_add_grid(D.grid, da.p, db.p, nullptr, s);
        SPK_HIP(hipMemcpyAsync(out, db.p, sizeof(double) * (size_t)no, hipMemcpyDeviceToHost, s));
    } else {
        dout.alloc((size_t)no, 16);
        if (stored) k::amg_restrict(D.R, da.p, db.p, dout.p, nullptr, s);
        else k::amg_restrict_grid(D.grid, da.p, db.p, dout.p, nullptr, s);
        SPK_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * (size_t)no, hipMemcpyDeviceToHost, s));
    }
    SPK_HIP(hipStreamSynchronize(s));
}

// the test hook of the level operators: one launch of either route on copies of the caller's vectors
void amg_debug_operator(spk_ctx *c, int l, int which, int stencil, double alpha, double beta, const double *x, const double *xo,
                        const double *b, double *out)
{
    AmgDev &d = *c->amg_d;
    if (l < 1 || l + 1 >= (int)d.lv.size())
        fail(SPK_ERR_ARG, "amg: operator hook: level %d is not between level 0 and the coarsest level %d", l, (int)d.lv.size() - 1);
    if (which < 0 || which > 3 || (stencil != 0 && stencil != 1)) fail(SPK_ERR_ARG, "amg: operator hook: which is 0..3, stencil 0 or 1");
    AmgLevelDev &D = d.lv[(size_t)l];
    if (stencil && !(d.info.coarsening == SPK_AMG_COARSEN_GRID && d.info.galerkin == SPK_AMG_GALERKIN_STENCIL && D.grid.on))
        fail(SPK_ERR_STATE, "amg: level %d was not built by -spk_mg_galerkin stencil: its pattern is no closed form", l);
    hipStream_t s = c->stream;
    const size_t n = (size_t)D.n;
    const bool step = which & 1, gated = which >= 2;
    DevBuf<double> dx, dxo, db, dout;
    DevBuf<int32_t> gate;
    dx.upload(x, n, 16);
    if (step) db.upload(b, n, 16);
    if (step && xo) dxo.upload(xo, n, 16);
    if (gated) {
        const int32_t one = 1;
        gate.upload(&one, 1);
        dout.upload(out, n, 16);
    } else {
        dout.alloc(n, 16);
    }
    const int32_t *done = gated ? gate.p : nullptr;
    const double *yo = step && xo ? dxo.p : nullptr;
    if (stencil) k::amg_stencil_op(D.A, D.grid.fd, D.grid.bs, step ? 1 : 0, dx.p, D.dinv.p, db.p, yo, dout.p, alpha, beta, done, s);
    else if (step) k::amg_cheb_csr(D.A, D.dinv.p, db.p, dx.p, yo, dout.p, alpha, beta, done, s);
    else k::amg_spmv(D.A, dx.p, dout.p, done, s);
    SPK_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    c->check_device_error();
}

// the test hook of the set-up's Lanczos: either route on one level of the device-built hierarchy as it stands (level 0:
// the context's layout and the D^-1 of its CSR copy, as at the build; no binade scale)
void amg_debug_lanczos(spk_ctx *c, int l, int resident, int32_t *steps, double *al, double *be)
{
    if (c->amg_h) fail(SPK_ERR_STATE, "amg: Lanczos hook: the hierarchy was built on the host -- pass -spk_gamg_setup device");
    AmgDev &d = *c->amg_d;
    if (l < 0 || l + 1 >= (int)d.lv.size()) fail(SPK_ERR_ARG, "amg: Lanczos hook: level %d has no Ritz estimate (levels: %d)", l, (int)d.lv.size());
    if (resident != 0 && resident != 1) fail(SPK_ERR_ARG, "amg: Lanczos hook: resident is 0 or 1");
    c->ensure_scratch();
    AmgLevelDev &D = d.lv[(size_t)l];
    DevBuf<double> dinv0;
    if (l == 0) {
        dinv0.alloc((size_t)c->n_local, 8);
        k::extract_diag_inv(c->Ad, dinv0.p, c->stream);
    }
    const CsrDev *M = l ? &D.A : nullptr;
    const int32_t n = l ? D.A.nrows : c->n_local;
    const int64_t nv = l ? n : c->ld;
    const double *dinv = l ? D.dinv.p : dinv0.p;
    double lmin = 0.0, lmax = 0.0;
    LzTri tri;
    LzWork work;
    if (resident) dev_lanczos_resident(c, work, M, n, nv, dinv, &lmin, &lmax, 1.0, nullptr, &tri);
    else dev_lanczos(c, M, n, nv, dinv, &lmin, &lmax, 1.0, nullptr, &tri);
    *steps = (int32_t)tri.al.size();
    std::copy(tri.al.begin(), tri.al.end(), al);
    std::copy(tri.be.begin(), tri.be.end(), be);
}

// the fine level's product runs in the row-type 2x2 layout (what a_mult takes for it) on one rank
// (n_local % 2: never false here -- the 2x2 blocked copy the row types are built over exists only for an even n_local;
// the condition states what amg_cheb_dict2 needs rather than guarding a case that occurs)
static bool fused_fine(const spk_ctx *c)
{
    return c->spmv_format != 0 && c->Adict.ok && c->Adict.bs == 2 && c->n_ghost == 0 && c->n_local % 2 == 0;
}

// nu smoothing steps on level l from *y (nullptr: the zero guess); returns the buffer holding the result
static double *smooth(spk_ctx *c, AmgLevelDev &D, int l, const double *b, double *y, const int32_t *done)
{
    hipStream_t s = c->stream;
    const double *dinv = l == 0 ? c->dinv.p : D.dinv.p;
    const double *prev = nullptr;   // the iterate before y (nullptr: zero)
    for (size_t k = 0; k < D.alpha.size(); ++k) {
        double *dst = y == D.ya.p ? D.yb.p : D.ya.p;   // may be `prev`: each entry is read before it is written
        if (l == 0 && y && fused_fine(c)) {   // the 2x2 row-type layout: product and step in one pass
            k::amg_cheb_dict2(c->Adict, dinv, b, y, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else if (l == 0) {                   // other layouts: the layout's own product, then a vector pass
            if (y) a_mult(c, y, D.t.p, nullptr, nullptr, done, false, nullptr);
            k::amg_cheb_vec(D.n, dinv, b, D.t.p, y, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else if (y && D.stencil_op) {
            k::amg_stencil_op(D.A, D.grid.fd, D.grid.bs, 1, y, dinv, b, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else if (y) {
            k::amg_cheb_csr(D.A, dinv, b, y, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else {
            k::amg_cheb_vec(D.n, dinv, b, nullptr, nullptr, nullptr, dst, D.alpha[k], 0.0, done, s);
        }
        prev = y;
        y = dst;
    }
    return y;
}

void amg_apply(spk_ctx *c, const double *x, double *y, int mode, const int32_t *done, const double **last)
{
    hipStream_t s = c->stream;
    AmgDev &d = *c->amg_d;
    const size_t L = d.lv.size();
    std::vector<double *> cur(L, nullptr);
    auto rhs = [&](size_t l) -> const double * { return l == 0 ? x : d.lv[l].b.p; };
    size_t run = 0;
    for (size_t i = 0; i < d.steps.size(); ++i) {   // the cycle's steps in order (amg_cycle_steps); under V: down, coarse, up
        if (run < d.runs.size() && (size_t)d.runs[run].first == i) {   // a tail run: one launch of one workgroup
            const size_t t = (size_t)d.info.tail_first;
            k::amg_tail(d.tail_desc.p, d.tail_stencil, (int32_t)d.runs[run].first, (int32_t)d.runs[run].second, done, s);
            cur[t] = d.run_sel[run] ? d.lv[t].yb.p : d.lv[t].ya.p;
            i = (size_t)d.runs[run++].second - 1;
            continue;
        }
        const size_t l = (size_t)d.steps[i].level;
        AmgLevelDev &D = d.lv[l];
        switch (d.steps[i].kind) {
        case SPK_AMG_STEP_PRE0: cur[l] = smooth(c, D, (int)l, rhs(l), nullptr, done); break;
        case SPK_AMG_STEP_PRE:
        case SPK_AMG_STEP_POST: cur[l] = smooth(c, D, (int)l, rhs(l), cur[l], done); break;
        case SPK_AMG_STEP_DOWN: {   // residual, restriction
            if (l == 0) a_mult(c, cur[l], D.t.p, nullptr, nullptr, done, false, nullptr);
            double *o = D.ya.p == cur[l] ? D.yb.p : D.ya.p;
            if (l > 0 && D.stencil_op) k::amg_stencil_op(D.A, D.grid.fd, D.grid.bs, 0, cur[l], nullptr, nullptr, nullptr, o, 0.0, 0.0, done, s);
            else if (l > 0) k::amg_spmv(D.A, cur[l], o, done, s);
            const double *t = l == 0 ? D.t.p : o;
            if (D.grid.matrix_free) k::amg_restrict_grid(D.grid, rhs(l), t, d.lv[l + 1].b.p, done, s);
            else k::amg_restrict(D.R, rhs(l), t, d.lv[l + 1].b.p, done, s);
            break;
        }
        case SPK_AMG_STEP_COARSE:   // exact coarse solve
            k::amg_dense(d.cinv.p, D.n, rhs(l), D.ya.p, done, s);
            cur[l] = D.ya.p;
            break;
        default:   // SPK_AMG_STEP_UP: prolongation + correction
            if (D.grid.matrix_free) k::amg_prolong_add_grid(D.grid, cur[l + 1], cur[l], done, s);
            else k::amg_prolong_add(D.P, cur[l + 1], cur[l], done, s);
        }
    }
    if (last) *last = cur[0];   // the caller's own pass reads the iterate where it lies
    else k::amg_out(mode, c->n_local, cur[0], y, done, s);
}

}  // namespace spk

// ---------------------------------------------------------------------------
// host-only entry points (no GPU)
// ---------------------------------------------------------------------------
extern "C" {

void spk_default_amg_opts(spk_amg_opts *o)
{
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->max_levels = 10;
    o->coarse_eq_limit = 50;
    o->nsmooths = 1;
    o->smoother = SPK_AMG_CHEBYSHEV;
    o->threshold = 0.0;
    o->smooth_its = 2;
    o->block_size = 0;
    o->esteig[0] = 0.0;
    o->esteig[1] = 0.1;
    o->esteig[2] = 0.0;
    o->esteig[3] = 1.1;
    o->richardson_scale = 1.0;
    o->setup = SPK_AMG_SETUP_HOST;
    o->lanczos = SPK_AMG_LANCZOS_STEPWISE;
}

#define SPK_HOST_TRY try {
#define SPK_HOST_CATCH                                                                   \
    }                                                                                    \
    catch (const spk::Error &e) { spk::set_create_error(e.msg); return e.code; }         \
    catch (const std::exception &e) { spk::set_create_error(e.what()); return SPK_ERR_NOMEM; } \
    return SPK_OK;

int spk_amg_build_host(int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, const spk_amg_opts *o,
                       spk_amg_hier **out)
{
    if (!out || !rowptr || !colidx || !val || !o || n <= 0) return SPK_ERR_ARG;
    *out = nullptr;
    SPK_HOST_TRY
    spk::HostCsr A;
    A.nrows = A.ncols = n;
    A.rp.assign(rowptr, rowptr + n + 1);
    A.ci.assign(colidx, colidx + rowptr[n]);
    A.v.assign(val, val + rowptr[n]);
    for (int32_t c : A.ci)
        if (c < 0 || c >= n) spk::fail(SPK_ERR_ARG, "amg: column %d outside [0,%d)", (int)c, (int)n);
    auto h = std::make_unique<spk_amg_hier>();
    spk::amg_build(h->h, std::move(A), *o);
    *out = h.release();
    SPK_HOST_CATCH
}

int spk_amg_refresh_host(spk_amg_hier *h, const double *val)
{
    if (!h || !val) return SPK_ERR_ARG;
    SPK_HOST_TRY
    spk::amg_refresh(h->h, val);
    SPK_HOST_CATCH
}

int spk_amg_destroy_host(spk_amg_hier *h)
{
    delete h;
    return SPK_OK;
}

int spk_amg_host_info(const spk_amg_hier *h, spk_amg_info *info)
{
    if (!h || !info) return SPK_ERR_ARG;
    *info = h->h.info;
    return SPK_OK;
}

int spk_amg_host_level(const spk_amg_hier *h, int level, int which, int32_t *nrows, int32_t *ncols, int64_t *nnz,
                       int32_t *rowptr, int32_t *colidx, double *val)
{
    if (!h) return SPK_ERR_ARG;
    SPK_HOST_TRY
    h->h.level(level, which, {nrows, ncols, nnz, rowptr, colidx, val});
    SPK_HOST_CATCH
}

int spk_amg_host_aggregates(const spk_amg_hier *h, int level, int32_t *nnodes, int32_t *agg)
{
    if (!h) return SPK_ERR_ARG;
    SPK_HOST_TRY
    spk::aggregates_out(h->h.lv, h->h.info, level, nnodes, agg);
    SPK_HOST_CATCH
}

int spk_amg_stencil_children(const int32_t *fine, const int32_t *coarse, int32_t node, int32_t *n, int32_t *nodes, double *weights)
{
    if (!fine || !coarse || !n) return SPK_ERR_ARG;
    SPK_HOST_TRY
    for (int a = 0; a < 3; ++a)
        if (fine[a] < 1 || (coarse[a] != fine[a] && coarse[a] != fine[a] / 2 + 1))
            spk::fail(SPK_ERR_ARG, "amg: %d coarse nodes are not a coarsening of %d fine ones", (int)coarse[a], (int)fine[a]);
    if (node < 0 || (int64_t)node >= (int64_t)coarse[0] * coarse[1] * coarse[2]) spk::fail(SPK_ERR_ARG, "amg: coarse node %d outside the grid", (int)node);
    *n = spk::galerkin_stencil_children(fine, coarse, node, nodes, weights);
    SPK_HOST_CATCH
}

int spk_amg_cycle_steps(int32_t levels, int32_t cycle, int64_t *nsteps, int32_t *steps)
{
    if (!nsteps) return SPK_ERR_ARG;
    SPK_HOST_TRY
    const std::vector<spk::AmgStep> st = spk::amg_cycle_steps(levels, cycle);
    *nsteps = (int64_t)st.size();
    for (size_t i = 0; steps && i < st.size(); ++i) steps[2 * i] = st[i].kind, steps[2 * i + 1] = st[i].level;
    SPK_HOST_CATCH
}

}  // extern "C"
