// spk_gs_stamps.hpp -- developer build `make GS_STAMPS=1`: phase time stamps of form 7's fused Gram-Schmidt launch
// (gs_fused_kernel).  Thread 0 of every workgroup records wall_clock64() (100 MHz, one counter for the whole device) at
// the points below; a launch writes the rows of its iteration `loc`, so after a solve the buffer holds, per loc, the
// last cycle's launch (read with spk_debug_gs_stamps, tabulated by tools/gs_phases.py).  The bodies the launch shares
// with the kernels of form 5 (mdot_tiles, maxpy_uhead_tiles) stamp through a pointer that only spk_k_iter.hip's copy of
// the variable below ever gets: in every other kernel file it stays null.  Without the flag GS_STAMP is empty and the
// object code is that of a build without this header.
#pragma once
#include <hip/hip_runtime.h>

namespace spk {
namespace k {

enum GsStamp {
    kGsEntry = 0,      // kernel entry
    kGsFirstLoads,     // the first tile's first group of loads returned (behind its sums)
    kGsTilesDone,      // VecMDot's tiles done
    kGsPublished,      // the workgroup's partials published
    kGsTotalsSeen,     // the totals this workgroup needs seen
    kGsPrologueDone,   // kernel B's scalar prologue done
    kGsBTilesDone,     // kernel B's tiles done
    kGsEntryRaw,       // where the entry stamp is taken; copied to kGsEntry once the gate has let the launch pass, so that a
                       // launch enqueued behind the end of a solve (gated off) leaves the rows of its loc alone
    kGsStampN = 8
};
constexpr int kGsStampLocs = 64, kGsStampWgs = 256;

#ifdef SPK_GS_STAMPS
static __device__ unsigned long long *gs_stamp_rows;   // one per kernel file; null except in spk_k_iter.hip during a solve
#define GS_STAMP(k_)                                                                                            \
    do {                                                                                                        \
        unsigned long long *gs_sb_ = ::spk::k::gs_stamp_rows;                                                   \
        if (gs_sb_ && threadIdx.x == 0) gs_sb_[(size_t)blockIdx.x * ::spk::k::kGsStampN + (k_)] = wall_clock64(); \
    } while (0)

#define GS_STAMP_COPY(to_, from_)                                                                               \
    do {                                                                                                        \
        unsigned long long *gs_sb_ = ::spk::k::gs_stamp_rows;                                                   \
        if (gs_sb_ && threadIdx.x == 0)                                                                         \
            gs_sb_[(size_t)blockIdx.x * ::spk::k::kGsStampN + (to_)] = gs_sb_[(size_t)blockIdx.x * ::spk::k::kGsStampN + (from_)]; \
    } while (0)

// host side (call from the file whose kernel stamps): points the next launch on s at the rows of iteration loc
static inline unsigned long long **gs_stamp_table()
{
    static unsigned long long *rows[kGsStampLocs] = {};
    if (!rows[0]) {
        unsigned long long *buf = nullptr;
        const size_t n = (size_t)kGsStampLocs * kGsStampWgs * kGsStampN;
        if (hipMalloc((void **)&buf, n * 8) != hipSuccess || hipMemset(buf, 0, n * 8) != hipSuccess) return nullptr;
        for (int l = 0; l < kGsStampLocs; ++l) rows[l] = buf + (size_t)l * kGsStampWgs * kGsStampN;
    }
    return rows;
}
static inline void gs_stamps_aim(int loc, int grid, hipStream_t s)
{
    unsigned long long **rows = gs_stamp_table();
    if (!rows || loc < 0 || loc >= kGsStampLocs || grid > kGsStampWgs) return;
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(gs_stamp_rows), &rows[loc], sizeof(rows[loc]), 0, hipMemcpyHostToDevice, s);
}
static inline bool gs_stamps_fetch(unsigned long long *out)   // kGsStampLocs x kGsStampWgs x kGsStampN
{
    unsigned long long **rows = gs_stamp_table();
    if (!rows) return false;
    return hipMemcpy(out, rows[0], (size_t)kGsStampLocs * kGsStampWgs * kGsStampN * 8, hipMemcpyDeviceToHost) == hipSuccess;
}
#else
#define GS_STAMP(k_) do { } while (0)
#define GS_STAMP_COPY(to_, from_) do { } while (0)
static inline void gs_stamps_aim(int, int, hipStream_t) {}
static inline bool gs_stamps_fetch(unsigned long long *) { return false; }
#endif

}  // namespace k
}  // namespace spk
