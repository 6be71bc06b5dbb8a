// gs_variant_check.cpp -- which instantiation form 7's fused Gram-Schmidt launch runs (csrc/spk_gs_launch.hpp:
// gs_fused_variant, gs_fused_grid, plane_class, dot_groups) on the shapes of tests/test_gpu_gs_*.py, without a GPU:
// rows and m of the assembled systems, n2 = (rows + m + 1) / 2 VecMDot's length in double2, its whole tiles and remainder
// those of 2048 double2 on a grid of 256.  Compiled with g++ and the sanitizers by tests/test_gs_variant_cpu.py.
#include <cstdint>
#include <cstdio>

#include "spk_gs_launch.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

using namespace spk::k;

struct Shape { const char *name; int64_t rows; int m; int64_t n2, whole, rem; bool staged; };

int main()
{
    const GsKnobs all{true, true, true};
    const Shape shapes[] = {
        {"1024 x 512 saddle", 1048576, 4, 524290, 256, 2, true},
        {"1024 x 512, K = A", 1048576, 0, 524288, 256, 0, false},
        {"915 x 573 saddle", 1048590, 4, 524297, 256, 9, true},
        {"1024 x 1024 saddle", 2097152, 4, 1048578, 512, 2, true},
        {"1025 x 1025 saddle", 2101250, 4, 1050627, 513, 3, false},     // whole tiles no multiple of the grid
        {"1030 x 1030 saddle", 2121800, 4, 1060902, 518, 38, false},    // and a long remainder
        {"128 x 128 x 32 saddle", 1572864, 6, 786435, 384, 3, false},   // whole tiles no multiple of the grid
    };
    for (const Shape &s : shapes) {
        const int64_t n2 = (s.rows + s.m + 1) / 2;
        CHECK(n2 == s.n2 && n2 / 2048 == s.whole && n2 % 2048 == s.rem);
        CHECK(gs_fused_grid(s.rows) == 256);
        if (gs_fused_variant(all, s.rows, n2, s.m, s.m == 4) != (s.staged ? kGsKeepAheadTail : kGsKeepAhead)) {
            std::printf("FAILED %s\n", s.name);
            ++failures;
        }
    }

    // below the fat shape (256 tiles of 2048 double2) there is no fused launch, and nothing to stage
    CHECK(gs_fused_grid(1048576) == 256 && gs_fused_grid(1048575) == 0 && gs_fused_grid(0) == 0);
    CHECK(gs_fused_variant(all, 1048574, 524289, 4, 1) == kGsKeepAhead);

    // the remainder's edges: kGsTailMax = 16 double2 are staged, 17 are a loop trip; none is none
    CHECK(kGsTailMax == 16);
    CHECK(gs_fused_variant(all, 1048576, 256 * 2048 + 1, 4, 1) == kGsKeepAheadTail);
    CHECK(gs_fused_variant(all, 1048576, 256 * 2048 + 16, 4, 1) == kGsKeepAheadTail);
    CHECK(gs_fused_variant(all, 1048576, 256 * 2048 + 17, 4, 1) == kGsKeepAhead);
    CHECK(gs_fused_variant(all, 1048576, 256 * 2048, 4, 1) == kGsKeepAhead);

    // the eight knob combinations on 1024 x 512 saddle: each knob counts only on top of the one before it
    for (int bits = 0; bits < 8; ++bits) {
        const GsKnobs k{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0};
        const GsVariant want = !k.keep ? kGsPlain : !k.ahead ? kGsKeep : !k.tail ? kGsKeepAhead : kGsKeepAheadTail;
        CHECK(gs_fused_variant(k, 1048576, 524290, 4, 1) == want);
    }

    // MP = 4 without parity planes has no registers for the loads ahead (and so no staged remainder); MP = 8 has
    CHECK(gs_fused_variant(all, 1048576, 524290, 3, 0) == kGsKeep);
    CHECK(gs_fused_variant(all, 1048576, 524290, 4, 0) == kGsKeep);
    CHECK(gs_fused_variant(all, 1048576, 524291, 6, 0) == kGsKeepAheadTail);
    CHECK(gs_fused_variant(GsKnobs{true, true, false}, 1048576, 524291, 6, 0) == kGsKeepAhead);

    CHECK(plane_class(0) == 0 && plane_class(1) == 4 && plane_class(4) == 4 && plane_class(5) == 8 && plane_class(8) == 8);
    CHECK(dot_groups(0) == 1 && dot_groups(1) == 1 && dot_groups(8) == 1 && dot_groups(9) == 2 && dot_groups(40) == 5);

    if (failures) {
        std::printf("%d gs variant checks FAILED\n", failures);
        return 1;
    }
    std::printf("all gs variant checks passed\n");
    return 0;
}
