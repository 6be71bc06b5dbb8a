// The device assembly kernels run on the CPU: the phase functions of csrc/spk_assembly_core.hpp -- the ones
// spk_k_assembly.hip and spk_k_assembly3d.hip call -- executed workgroup by workgroup, phase by phase, thread 0..255 in
// turn, with the output arrays and the workgroup's LDS arrays allocated at exactly their sizes (the sanitizers see every
// access), and the result compared with the host assembler byte for byte.
//
// Cases on stdin, one per line:  <2|3> mx my mz row_begin row_end apply_bc <file of kappa as raw doubles | ->
// (mz is 0 for the 2-D grid).  Prints one line per failure and a summary; exit status 0 when every case passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "spk.h"
#include "spk_assembly.h"
#include "spk_assembly_core.hpp"

namespace as = spk::assembly;

namespace {

constexpr int kThreads = 256;   // the kernels' workgroup size

template <class T>
std::unique_ptr<T[]> exact(size_t n, int fill)
{
    std::unique_ptr<T[]> p(new T[n]);
    std::memset(p.get(), fill, n * sizeof(T));
    return p;
}

// what a workgroup finds in LDS when it starts: nothing it may use
void poison(double *p, int n)
{
    for (int i = 0; i < n; ++i) p[i] = std::nan("");
}

struct Slab {
    int64_t n, nnz;
    std::unique_ptr<int32_t[]> rowptr, colidx;
    std::unique_ptr<double[]> val, f;
    Slab(int64_t n_, int64_t nnz_, int fill)
        : n(n_), nnz(nnz_), rowptr(exact<int32_t>((size_t)n_ + 1, fill)), colidx(exact<int32_t>((size_t)nnz_, fill)),
          val(exact<double>((size_t)nnz_, fill)), f(exact<double>((size_t)n_, fill))
    {
    }
    bool same(const Slab &o) const
    {
        return !std::memcmp(rowptr.get(), o.rowptr.get(), sizeof(int32_t) * ((size_t)n + 1)) &&
               !std::memcmp(colidx.get(), o.colidx.get(), sizeof(int32_t) * (size_t)nnz) &&
               !std::memcmp(val.get(), o.val.get(), sizeof(double) * (size_t)nnz) && !std::memcmp(f.get(), o.f.get(), sizeof(double) * (size_t)n);
    }
};

bool run2(int mx, int my, int64_t rb, int64_t re, int bc, const double *kappa)
{
    const int64_t nnz = SpkAssemblySlabNnz(mx, my, rb, re);
    if (nnz < 0) return false;
    Slab dev(re - rb, nnz, 0x5a), host(re - rb, nnz, 0xa5);
    if (SpkAssembleOperator_LaplaceKappa(mx, my, rb, re, kappa, host.rowptr.get(), host.colidx.get(), host.val.get(), host.f.get(), bc, 2) != SPK_OK)
        return false;
    const int j0 = (int)(rb / (2 * mx)), j1 = (int)(re / (2 * mx)), nstrips = as::strips2(mx);
    auto Ke = exact<double>(as::kLdsKe2, 0), Fe = exact<double>(as::kLdsFe2, 0), G = exact<double>(as::kLdsG2, 0),
         kap = exact<double>(as::kLdsKap2, 0);
    for (int64_t b = 0; b < as::grid2(mx, j0, j1); ++b) {
        poison(Ke.get(), as::kLdsKe2), poison(Fe.get(), as::kLdsFe2), poison(G.get(), as::kLdsG2), poison(kap.get(), as::kLdsKap2);
        for (int t = 0; t < kThreads; ++t) as::asm2_phase1a(t, kThreads, (unsigned)b, mx, my, j0, nstrips, kappa, G.get(), kap.get());
        for (int t = 0; t < kThreads; ++t) as::asm2_phase1b(t, kThreads, (unsigned)b, mx, my, j0, nstrips, G.get(), kap.get(), Ke.get(), Fe.get());
        for (int t = 0; t < kThreads; ++t)
            as::asm2_phase2(t, kThreads, (unsigned)b, mx, my, j0, j1, nstrips, bc, Ke.get(), Fe.get(), dev.rowptr.get(), dev.colidx.get(),
                            dev.val.get(), dev.f.get());
    }
    return dev.same(host);
}

bool run3(int mx, int my, int mz, int64_t rb, int64_t re, int bc, const double *kappa)
{
    const int64_t nnz = SpkAssemblySlabNnz3D(mx, my, mz, rb, re);
    if (nnz < 0) return false;
    Slab dev(re - rb, nnz, 0x5a), host(re - rb, nnz, 0xa5);
    if (SpkAssembleOperator_Laplace3DKappa(mx, my, mz, rb, re, kappa, host.rowptr.get(), host.colidx.get(), host.val.get(), host.f.get(), bc,
                                           2) != SPK_OK)
        return false;
    const int64_t plane = (int64_t)3 * mx * my;
    const int k0 = (int)(rb / plane), k1 = (int)(re / plane), nstrips = as::strips3(mx);
    auto G = exact<double>(as::kLdsG3, 0), Kv = exact<double>(as::kLdsKv3, 0);
    for (int64_t b = 0; b < as::grid3(mx, my, k0, k1); ++b) {
        poison(G.get(), as::kLdsG3), poison(Kv.get(), as::kLdsKv3);
        for (int t = 0; t < kThreads; ++t) as::asm3_phase1(t, kThreads, (unsigned)b, mx, my, mz, k0, nstrips, kappa, G.get());
        for (int t = 0; t < kThreads; ++t) as::asm3_phase2a(t, kThreads, (unsigned)b, mx, my, mz, k0, nstrips, G.get(), Kv.get());
        for (int t = 0; t < kThreads; ++t)
            as::asm3_phase2b(t, kThreads, (unsigned)b, mx, my, mz, k0, k1, nstrips, bc, G.get(), Kv.get(), dev.rowptr.get(), dev.colidx.get(),
                             dev.val.get(), dev.f.get());
    }
    return dev.same(host);
}

}  // namespace

int main()
{
    int cases = 0, failed = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int dim, mx, my, mz, bc;
        long long rb, re;
        std::string kfile;
        if (!(in >> dim >> mx >> my >> mz >> rb >> re >> bc >> kfile) || (dim != 2 && dim != 3) || mx < 2 || my < 2 || (dim == 3 && mz < 2)) {
            std::printf("bad case line: %s\n", line.c_str());
            return 2;
        }
        const size_t ne = (size_t)(mx - 1) * (my - 1) * (dim == 3 ? mz - 1 : 1);
        std::unique_ptr<double[]> kappa;
        if (kfile != "-") {
            kappa = exact<double>(ne, 0);
            std::ifstream kf(kfile, std::ios::binary);
            if (!kf.read(reinterpret_cast<char *>(kappa.get()), (std::streamsize)(ne * sizeof(double)))) {
                std::printf("cannot read %zu values of kappa from %s\n", ne, kfile.c_str());
                return 2;
            }
        }
        ++cases;
        const bool ok = dim == 2 ? run2(mx, my, rb, re, bc, kappa.get()) : run3(mx, my, mz, rb, re, bc, kappa.get());
        if (!ok) {
            ++failed;
            std::printf("MISMATCH: %s\n", line.c_str());
        }
    }
    std::printf("%d cases, %d failed\n", cases, failed);
    if (cases > 0 && failed == 0) std::printf("all assembly kernel host checks passed\n");
    return cases > 0 && failed == 0 ? 0 : 1;
}
