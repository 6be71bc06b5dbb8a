// spk_gs_launch.hpp -- which instantiation form 7's fused Gram-Schmidt launch runs (spk_k_iter.hip gs_fused_kernel,
// gs_fused_tail_kernel): its constants, its template arguments and the choice between its variants as pure functions
// of a few integers.  No HIP types: host code, compiles with plain g++ (tests/host/gs_variant_check.cpp).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace spk {
namespace k {

constexpr int kVecMaxBlocks = 256;   // grid of the reducing vector kernels on big vectors: one fat workgroup per CU
constexpr int kGsT = 512, kGsU = 4, kGsG = 4;   // vec_shape's fat shape (mdot_kernel<NG, 512, 4, true, 4>, kernel B <512, 4, 4, MP>)

// What a launch with a keep set asks for ahead of the totals wait beyond V_4 .. V_7 (SPK_GS_AHEAD; NoKeep in
// spk_device.hpp): kGsAhead[MP / 4][NG - 1] vectors of the group V_8 .. V_11, held across the wait in the registers
// of the tile loop's buffer, 16 each.  Sized by the compiler's resource remark (tests/test_gs_resources_cpu.py
// reads this table and the remark of every instantiation): MP = 4 takes the registers of the two planes that parity
// planes leave unused (KeepSet::PK) and still spills 4 .. 12 VGPRs with the whole group, so it holds three vectors.
constexpr int kGsAhead[3][5] = {
    {4, 4, 4, 4, 4},   // MP = 0
    {3, 3, 3, 3, 3},   // MP = 4
    {4, 4, 4, 4, 4},   // MP = 8
};

// The short remainder tile of form 7's launch (TAIL; gs_fused_tail_kernel, SPK_GS_TAIL): at most kGsTailMax double2 behind
// the whole tiles (at 1024^2 with the full Schur preconditioner the four multiplier entries), staged in LDS at entry
// instead of being a tile-loop trip of their own.  kGsTailSrc sources: w~ and the <= 40 vectors or planes of one
// reduction (GsArgs::cnt); 41 x 16 double2 = 10 496 B of the 19 776 B that LDS has free beside the keep set
// (160 KiB - 4 x 32 KiB - 12 992 B).
constexpr int kGsTailMax = 16, kGsTailSrc = 41;

// The MP template argument of kernel B's bodies: no planes of B D, up to four, up to eight
constexpr int plane_class(int m) { return m == 0 ? 0 : m <= 4 ? 4 : 8; }
// The NG template argument of VecMDot's bodies: groups of eight dot products (cnt <= 40: 1 .. 5)
constexpr int dot_groups(int cnt) { return cnt > 8 ? (cnt + 7) / 8 : 1; }

// The launch's grid for nl local rows; 0: not the fat vector shape
constexpr int64_t gs_fused_grid(int64_t nl)
{
    return nl / 2 < (int64_t)kVecMaxBlocks * kGsT * kGsU ? 0 : kVecMaxBlocks;   // >= 256 tiles of 2048 double2: both kernels' grids
}

// Test knobs, all on by default ("0" turns one off; SPK_GS_AHEAD=2 once added groups left to the L2: taken out,
// DESIGN.md 4, and runs as 1).  Read per solve, so that a test can flip one between two solves of one context.
struct GsKnobs {
    bool keep;    // the first tile's operands stay on chip between the launch's two passes
    bool ahead;   // with keep: a second group of basis loads is requested ahead of the totals wait
    bool tail;    // with both: a short remainder tile is staged in LDS at entry instead of being a tile-loop trip
};
inline GsKnobs gs_knobs_env()
{
    const auto on = [](const char *e) { return !(e && !strcmp(e, "0")); };
    return GsKnobs{on(getenv("SPK_GS_KEEP")), on(getenv("SPK_GS_AHEAD")), on(getenv("SPK_GS_TAIL"))};
}

enum GsVariant {
    kGsPlain,           // gs_fused_kernel<NG, MP, false>
    kGsKeep,            // gs_fused_kernel<NG, MP, true>
    kGsKeepAhead,       // gs_fused_kernel<NG, MP, true, kGsAhead>
    kGsKeepAheadTail,   // gs_fused_tail_kernel<NG, MP, kGsAhead>
};

// The variant of one launch: nl local rows, MDot's length n2 in double2 (the multiplier entries included), m planes of
// B D, parity planes or not.  MP = 4: the loads ahead of the wait take the registers of half the planes, which parity
// planes leave free (KeepSet::PK); rows of B D that do not pack run the launch without them.  The remainder is staged
// where it is 1 .. kGsTailMax double2 behind whole tiles that are a multiple of the grid -- so that it would be a trip
// of its own beyond every workgroup's whole tiles.  Any other shape keeps the loop trip.
constexpr GsVariant gs_fused_variant(GsKnobs k, int64_t nl, int64_t n2, int m, int packed)
{
    if (!k.keep) return kGsPlain;
    if (!k.ahead || (plane_class(m) == 4 && !packed)) return kGsKeep;
    const int64_t grid = gs_fused_grid(nl), tile2 = (int64_t)kGsT * kGsU, whole = n2 / tile2, rem = n2 % tile2;
    const bool staged = k.tail && grid && rem > 0 && rem <= kGsTailMax && whole >= grid && whole % grid == 0;
    return staged ? kGsKeepAheadTail : kGsKeepAhead;
}

}  // namespace k
}  // namespace spk
