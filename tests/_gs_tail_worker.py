"""Cases of tests/test_gpu_gs_tail.py and the child process that runs all of them under one SPK_GS_TAIL:

    SPK_GS_TAIL=0|1 python _gs_tail_worker.py OUT_DIR      (a fresh process per variant: clean contexts)

The case loop, the pair of solves per case and the gated sequence behind "full" are tests/_gs_rig.py's; this child adds
Context.gs_launch() to the record of every solve: how many of form 7's launches staged their remainder tile in LDS.
Nothing here is imported by the CPU suite."""
import contextlib
import os
import sys

import _gs_rig as R
from _gs_rig import FULL, LOWER

TILE2, GRID, R_MAX = 2048, 256, 16   # the fused launch's tile (512 threads x 4 double2), its grid, kGsTailMax

# name: (grid, saddle, fact, restart, max_it).  1024 x 512 is the smallest fat vector: one whole tile per workgroup and
# the remainder of two double2 (the four multiplier entries) behind them; every max_it ends inside a restart cycle, so the
# launches enqueued behind the end of the solve pass through the staging gated off.
CASES = {
    "full": ((1024, 512), True, FULL, 30, 45),
    # nv crosses the edges of the groups of four with the epilogue's guards (and the cycle's last launch, dead_out)
    "restart4": ((1024, 512), True, FULL, 4, 9),
    "restart8": ((1024, 512), True, FULL, 8, 17),
    "restart9": ((1024, 512), True, FULL, 9, 19),
    "restart12": ((1024, 512), True, FULL, 12, 25),
    "restart13": ((1024, 512), True, FULL, 13, 27),
    "lower": ((1024, 512), True, LOWER, 30, 45),
    "jacobi": ((1024, 512), False, FULL, 30, 45),          # K = A: no remainder, the path must not engage
    # 915 x 573 = 256 x 2048 + 7 nodes: a remainder of nine double2, seven of them real nodes of the grid
    "real_nodes": ((915, 573), True, FULL, 30, 20),
    # 513 whole tiles and three double2 (one real node): the remainder is one of workgroup 1's ordinary trips -- loop trip
    "odd_1025": ((1025, 1025), True, FULL, 30, 12),
    "partial_tile": ((1030, 1030), True, FULL, 30, 12),    # a remainder of 38 double2 > kGsTailMax: loop trip
    "six_rows_3d": ((128, 128, 32), True, FULL, 30, 12),   # 384 whole tiles, no multiple of the grid: loop trip
}


def tail_expected(n, m):
    """The launcher's condition (gs_fused_variant in csrc/spk_gs_launch.hpp, stated again here) for n rows and m multipliers
    on the default launch."""
    n2 = (n + m + 1) // 2
    whole, rem = divmod(n2, TILE2)
    return 0 < rem <= R_MAX and whole >= GRID and whole % GRID == 0


def _record(c, info):
    launches, tail = c.gs_launch()
    return dict(R._record(None, info, c.iteration_form()[0]), launches=int(launches), tail=int(tail))


def main(out_dir):
    S = R.package()
    res = {"knob": os.environ.get("SPK_GS_TAIL")}
    with contextlib.ExitStack() as stack:
        for _ in R.solved_cases(S, CASES, stack, out_dir, res, _record):
            pass


if __name__ == "__main__":
    main(sys.argv[1])
