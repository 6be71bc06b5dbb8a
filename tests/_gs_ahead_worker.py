"""Cases of tests/test_gpu_gs_ahead.py and the child process that runs all of them under one SPK_GS_AHEAD:

    SPK_GS_AHEAD=0|1|2 python _gs_ahead_worker.py OUT_DIR      (a fresh process per variant: clean contexts)

The case loop, the pair of solves per case and the gated sequence behind "full" are tests/_gs_rig.py's; the solves under a
wait bound of one tick behind them are this child's own.  Nothing here is imported by the CPU suite."""
import contextlib
import os
import sys

import numpy as np

import _gs_rig as R
from _gs_rig import FULL, GSF, LOWER, _record

# name: (grid, saddle, fact, restart, max_it).  1024 x 512 is the smallest fat vector: one tile per workgroup, workgroup 0
# with the multiplier tail tile; restart 30 with 45 iterations takes nv past 4, 5, 8, 9, 12, 13 (the edges of the kept
# group, the two groups requested ahead of the totals wait and the one behind them) and half-way through them again.
CASES = {
    "full": ((1024, 512), True, FULL, 30, 45),
    # cycles whose last launch has a partly or wholly dead second group ahead (dead_out in play)
    "restart4": ((1024, 512), True, FULL, 4, 9),
    "restart8": ((1024, 512), True, FULL, 8, 17),
    "restart9": ((1024, 512), True, FULL, 9, 19),
    "restart12": ((1024, 512), True, FULL, 12, 25),
    "lower": ((1024, 512), True, LOWER, 30, 45),
    "jacobi": ((1024, 512), False, FULL, 30, 45),   # K = A: MP = 0
    "two_tiles": ((1024, 1024), True, FULL, 30, 33),      # the second tile takes the ordinary path
    "partial_tile": ((1030, 1030), True, FULL, 30, 12),   # a partial last tile; some workgroups have three tiles
    "six_rows_3d": ((128, 128, 32), True, FULL, 30, 12),  # m = 6: MP = 8
}


def main(out_dir):
    S = R.package()
    res = {"knob": os.environ.get("SPK_GS_AHEAD")}
    with contextlib.ExitStack() as stack:
        for name, c, rhs, x7, restart, max_it in R.solved_cases(S, CASES, stack, out_dir, res):
            if name != "full":
                continue
            # the bounded waits, one tick: SPK_ERR_HIP, then a clean solve with the same bits
            w = {"code": None, "message": ""}
            c.debug_set_wait_bound(1)
            try:
                c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart, iteration_form=GSF)
            except S.SpkError as e:
                w = {"code": int(e.code), "message": str(e)}
            c.debug_set_wait_bound(0)
            xb, ib = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart, iteration_form=GSF)
            w["after"] = _record(xb, ib, c.iteration_form()[0])
            w["after_x_equal"] = bool(np.array_equal(xb, x7))
            res["wait"] = w


if __name__ == "__main__":
    main(sys.argv[1])
