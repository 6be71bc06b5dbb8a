// spk_amg.hpp -- multigrid: the data of the host hierarchy and what spk_amg_host.cpp builds and refreshes it with.
// Host-pure: the standard library and include/spk.h only (the device copy is AmgDev, spk_internal.hpp).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/spk.h"

namespace spk {

// host CSR, columns sorted within each row
struct HostCsr {
    int32_t nrows = 0, ncols = 0;
    std::vector<int32_t> rp{0}, ci;
    std::vector<double> v;
    int64_t nnz() const { return (int64_t)ci.size(); }
};

// where a test hook copies one matrix to; any pointer may be null
struct CsrOut {
    int32_t *nrows, *ncols;
    int64_t *nnz;
    int32_t *rowptr, *colidx;
    double *val;
    void sizes(int32_t nr, int32_t nc, int64_t nz) const { if (nrows) *nrows = nr; if (ncols) *ncols = nc; if (nnz) *nnz = nz; }
};

struct AmgLevel {
    HostCsr A;              // A_l
    HostCsr Ptent, P, R;    // to level l+1 (empty on the coarsest level); R = P^T
    std::vector<double> dinv;
    std::vector<int32_t> agg;   // aggregate of every node (-1: isolated)
    double lo = 0.0, hi = 0.0;  // Chebyshev interval
};

struct AmgHier {
    spk_amg_opts o{};
    std::vector<AmgLevel> lv;
    std::vector<double> cinv;   // dense inverse of the coarsest A, row-major
    spk_amg_info info{};        // as the set-up loop filled it (setup_seconds: the host build)
    double dinv_sum = 0.0;      // sum |D_0^-1| at the build: its binade is the refresh's reference (amg_refresh)
    std::vector<int32_t> perm;  // sorted position of level 0 -> index in the CSR arrays the caller gave (amg_refresh)
    void level(int l, int which, const CsrOut &out) const;   // copy one matrix of a level out (see spk_get_amg_level)
};

// throws spk::Error
// host_builder: spk_amg_build_host's check -- it takes a set-up route and a Lanczos route it does not read
void amg_check_opts(const spk_amg_opts &o, bool host_builder = false);
// every field that decides the hierarchy agrees (all but cycle, tail, tail_rows and op, which steer the application);
// and those four taken from src
bool amg_same_hierarchy_opts(const spk_amg_opts &a, const spk_amg_opts &b);
void amg_take_application_opts(spk_amg_opts &dst, const spk_amg_opts &src);
void amg_build(AmgHier &h, HostCsr A, const spk_amg_opts &o);
// new values (in the order of the arrays amg_build was given) on the kept aggregates, prolongators and patterns: every
// A_l, D_l^-1, interval and the coarse inverse again.  A throw leaves h empty.
void amg_refresh(AmgHier &h, const double *val);

}  // namespace spk

struct spk_amg_hier {
    spk::AmgHier h;
};
