"""Cases of tests/test_gpu_gs_tail.py and the child process that runs all of them under one SPK_GS_TAIL:

    SPK_GS_TAIL=0|1 python _gs_tail_worker.py OUT_DIR      (a fresh process per variant: clean contexts)

Per case the child solves with AUTO (form 7 asserted by the test) and with forced form 5 on one context, compares the
two in place and writes the AUTO solve's x as OUT_DIR/<case>.npy and everything else to OUT_DIR/results.json (the
residual histories as hex floats: bit-exact; Context.gs_launch() of either solve: how many of form 7's launches staged
their remainder tile in LDS).  Nothing here is imported by the CPU suite."""
import contextlib
import json
import os
import sys

import numpy as np

UN3, GSF = 5, 7
LOWER, FULL = 1, 3
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
    """The launcher's condition (spk_k_iter.hip gs_fused_tail) for n rows and m multipliers on the default launch."""
    n2 = (n + m + 1) // 2
    whole, rem = divmod(n2, TILE2)
    return 0 < rem <= R_MAX and whole >= GRID and whole % GRID == 0


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


def _record(c, info):
    launches, tail = c.gs_launch()
    return {"its": int(info["its"]), "reason": int(info["reason"]), "form": int(c.iteration_form()[0]),
            "launches": int(launches), "tail": int(tail), "history": _hex(info["history"])}


def main(out_dir):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import saddle_point_petsc_amd as S

    res = {"tail": os.environ.get("SPK_GS_TAIL")}
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
            r = _record(c, i7)
            r["rows"], r["m"] = int(A.nrows), 0 if B is None else int(B.nrows)
            x5, i5 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart, iteration_form=UN3)
            r["form5"] = _record(c, i5)
            r["x_equals_form5"] = bool(np.array_equal(x7, x5))
            np.save(os.path.join(out_dir, name + ".npy"), x7)
            res[name] = r
            if name != "full":
                continue
            # -ksp_max_it in the middle of the second cycle, the convergence test live: the launches enqueued behind the end
            # of the solve are gated off with the remainder's loads in flight; the next solve must not notice
            _, ig = c.fgmres(rhs, rtol=1e-30, max_it=47, restart=restart)
            g = _record(c, ig)
            xa, ia = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart)
            g["after"] = _record(c, ia)
            g["after_x_equal"] = bool(np.array_equal(xa, x7))
            res["gated"] = g
    with open(os.path.join(out_dir, "results.json"), "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main(sys.argv[1])
