#!/usr/bin/env python3
"""Pipelined CG (spk_pipecg) and pipelined CG with residual replacement (spk_pipecgrr) on K = A against MINRES + Jacobi
and FGMRES(30) + gamg on one GPU, in one process:
    python tools/pipecg_bench.py [--grids 256 512 1024] [--its 300] [--rtol 1e-8] [--pipecg-only] [--rr] [--rr-only]
Per grid: pipecg with Jacobi (both norms), none and gamg; MINRES with Jacobi; FGMRES(30) with gamg; with --rr also
pipecgrr with Jacobi, none and gamg in both norms, with its replacements (the fixed-count runs set a tau that never
replaces, so their us per iteration carry the gap check alone).  Per row: us per
iteration over a fixed iteration count, iterations and solve time to rtol, the true relative residual; for pipecg
with a diagonal PC also the byte model of one iteration (the product in the layout it streams plus the vector
streams of the pass: 15 with Jacobi, 13 without a PC) and its fraction of 8 TB/s.  One JSON line per row."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import saddle_point_petsc_amd as S  # noqa: E402

PEAK = 8.0e12
STREAMS = {"jacobi": 15, "none": 13}   # pass: n z w s p x r (dinv) read, z s p x r w (m) written

ap = argparse.ArgumentParser()
ap.add_argument("--grids", type=int, nargs="+", default=[256, 512, 1024])
ap.add_argument("--its", type=int, default=300, help="iterations of the fixed-count runs (us per iteration)")
ap.add_argument("--rtol", type=float, default=1e-8)
ap.add_argument("--max-it", type=int, default=20000)
ap.add_argument("--pipecg-only", action="store_true", help="pipecg + Jacobi at the first grid only (a short kernel trace)")
ap.add_argument("--rr", action="store_true", help="pipecgrr rows as well")
ap.add_argument("--rr-only", action="store_true", help="pipecgrr + Jacobi at the first grid only (a short kernel trace)")
a = ap.parse_args()


def ctx(A, pc):
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    if pc == "gamg":
        c.pc_setup(S.PC_JACOBI, amg=True)
    else:
        c.pc_setup(S.PC_JACOBI if pc == "jacobi" else S.PC_NONE)
    return c


def run(c, solver, f, grid, pc, norm="unpreconditioned", **extra):
    solve = {"pipecg": c.pipecg, "minres": c.minres, "pipecgrr": c.pipecgrr}.get(solver)
    kw = dict(norm=norm) if solve else dict(restart=30)
    solve = solve or c.fgmres
    solve(f, rtol=0.0, abstol=0.0, max_it=20, **kw)   # warm-up: first-use allocations
    fixed_kw = dict(kw, tau=1e30) if solver == "pipecgrr" else kw   # pipecgrr: the check runs, no replacement
    _, fixed = solve(f, rtol=0.0, abstol=0.0, max_it=a.its, **fixed_kw)
    if solver == "pipecgrr":
        kw["tau"] = S.PIPECGRR_TAU_DEFAULT
    us = fixed["solve_seconds"] / fixed["its"] * 1e6
    x, conv = solve(f, rtol=a.rtol, max_it=a.max_it, **kw)
    true = np.linalg.norm(f - c.mult(x)) / np.linalg.norm(f)
    row = dict(grid=grid, solver=solver, pc=pc, norm=norm if solver != "fgmres" else "unpreconditioned",
               us_per_it=round(us, 2), its=conv["its"], reason=conv["reason"], cycles=conv["cycles"],
               seconds=round(conv["solve_seconds"], 5), true_rel_res=float(true), **extra)
    if solver == "pipecgrr":
        row.update(replacements=conv["replacements"], tau=kw["tau"])
    if solver == "pipecg" and pc in STREAMS:
        nbytes = c.spmv_info()["layout_bytes"] + STREAMS[pc] * 8 * c.sizes()["n_local"]
        row.update(model_bytes=nbytes, vector_streams=STREAMS[pc], tb_s=round(nbytes / us * 1e-6, 3),
                   frac_peak=round(nbytes / (us * 1e-6) / PEAK, 3))
    print(json.dumps(row), flush=True)


for grid in a.grids[:1] if a.rr_only else []:
    A, f = S.AssembleOperator_Laplace(grid)
    with ctx(A, "jacobi") as c:
        run(c, "pipecgrr", f, grid, "jacobi")
for grid in [] if a.rr_only else a.grids[:1] if a.pipecg_only else a.grids:
    A, f = S.AssembleOperator_Laplace(grid)
    with ctx(A, "jacobi") as c:
        for norm in (("unpreconditioned",) if a.pipecg_only else ("unpreconditioned", "natural")):
            run(c, "pipecg", f, grid, "jacobi", norm)
        if not a.pipecg_only:
            run(c, "minres", f, grid, "jacobi")
    if a.pipecg_only:
        break
    with ctx(A, "none") as c:
        run(c, "pipecg", f, grid, "none")
    with ctx(A, "gamg") as c:
        setup = c.amg_info()["setup_seconds"]
        run(c, "pipecg", f, grid, "gamg", amg_setup_seconds=round(setup, 3))
        run(c, "fgmres", f, grid, "gamg", amg_setup_seconds=round(setup, 3))
    if a.rr:
        for pc in ("jacobi", "none", "gamg"):
            with ctx(A, pc) as c:
                for norm in ("unpreconditioned", "natural"):
                    run(c, "pipecgrr", f, grid, pc, norm)
