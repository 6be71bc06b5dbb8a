// spk_amg.hpp -- smoothed-aggregation multigrid: the host hierarchy (spk_amg.cpp) and its device copy.
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

struct AmgLevel {
    HostCsr A;              // A_l
    HostCsr Ptent, P, R;    // to level l+1 (empty on the coarsest level); R = P^T
    std::vector<double> dinv;
    std::vector<int32_t> agg;   // aggregate of every node (-1: isolated)
    double lmin = 0.0, lmax = 0.0;
    double lo = 0.0, hi = 0.0;  // Chebyshev interval
};

struct AmgHier {
    spk_amg_opts o{};
    int bs = 1;
    std::vector<AmgLevel> lv;
    std::vector<double> cinv;   // dense inverse of the coarsest A, row-major
    double setup_seconds = 0.0;
    void info(spk_amg_info *out) const;
    // copy one matrix of a level out (see spk_get_amg_level)
    void level(int l, int which, int32_t *nrows, int32_t *ncols, int64_t *nnz, int32_t *rowptr, int32_t *colidx,
               double *val) const;
};

// throws spk::Error
void amg_check_opts(const spk_amg_opts &o);
void amg_build(AmgHier &h, HostCsr A, const spk_amg_opts &o);

}  // namespace spk

struct spk_amg_hier {
    spk::AmgHier h;
};
