"""Cases of tests/test_gpu_gs_ahead.py and the child process that runs all of them under one SPK_GS_AHEAD:

    SPK_GS_AHEAD=0|1|2 python _gs_ahead_worker.py OUT_DIR      (a fresh process per variant: clean contexts)

Per case the child solves with AUTO (form 7 asserted by the test) and with forced form 5 on one context, compares the
two in place and writes the AUTO solve's x as OUT_DIR/<case>.npy and everything else to OUT_DIR/results.json (the
residual histories as hex floats: bit-exact).  Nothing here is imported by the CPU suite."""
import contextlib
import json
import os
import sys

import numpy as np

UN3, GSF = 5, 7
LOWER, FULL = 1, 3

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


def _system(S, grid, saddle):
    if len(grid) == 3:
        A, f = S.AssembleOperator_Laplace3D(*grid, nthreads=16)
        B, g = S.AssembleOperator_Constraints3D(*grid)
        return A, B, np.concatenate([f, g])
    A, f = S.AssembleOperator_Laplace(*grid)
    if not saddle:
        return A, None, f
    B, g = S.AssembleOperator_Constraints(*grid)
    return A, B, np.concatenate([f, g])


def _ctx(S, A, B, fact):
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    if B is not None:
        c.set_block(S.BLOCK_A10, B)
    c.pc_setup(S.PC_SCHUR if B is not None else S.PC_JACOBI, fact)
    return c


def _hex(h):
    return [float(v).hex() for v in np.asarray(h, float)]


def _record(x, info, form):
    return {"its": int(info["its"]), "reason": int(info["reason"]), "form": int(form), "history": _hex(info["history"])}


def main(out_dir):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import saddle_point_petsc_amd as S

    res = {"ahead": os.environ.get("SPK_GS_AHEAD")}
    sys_key = ctx_key = None
    with contextlib.ExitStack() as stack:
        for name, (grid, saddle, fact, restart, max_it) in CASES.items():   # consecutive cases share system and context
            if (grid, saddle) != sys_key:
                stack.close()
                ctx_key = None
                sys_key = (grid, saddle)
                A, B, rhs = _system(S, grid, saddle)
            if (sys_key, fact) != ctx_key:
                stack.close()
                ctx_key = (sys_key, fact)
                c = stack.enter_context(_ctx(S, A, B, fact))
            x7, i7 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart)
            r = _record(x7, i7, c.iteration_form()[0])
            x5, i5 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart, iteration_form=UN3)
            r["form5"] = _record(x5, i5, c.iteration_form()[0])
            r["x_equals_form5"] = bool(np.array_equal(x7, x5))
            np.save(os.path.join(out_dir, name + ".npy"), x7)
            res[name] = r
            if name != "full":
                continue
            # -ksp_max_it in the middle of the second cycle: the launches enqueued behind the end of the solve are gated
            # off and return with their loads ahead of the wait in flight; the next solve must not notice
            _, ig = c.fgmres(rhs, rtol=1e-30, max_it=47, restart=restart)
            g = _record(None, ig, c.iteration_form()[0])
            xa, ia = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart)
            g["after"] = _record(xa, ia, c.iteration_form()[0])
            g["after_x_equal"] = bool(np.array_equal(xa, x7))
            res["gated"] = g
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
    with open(os.path.join(out_dir, "results.json"), "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main(sys.argv[1])
