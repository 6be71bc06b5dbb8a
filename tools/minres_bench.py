#!/usr/bin/env python3
"""MINRES (spk_minres) against FGMRES on one GPU, in one process:
    python tools/minres_bench.py [--grid 1024] [--its 300] [--rtol 1e-8]
Two systems: the saddle system with Schur DIAG (FGMRES: Schur FULL, today's default) and K = A with Jacobi (FGMRES:
Jacobi).  Per system and MINRES norm: us per iteration over a fixed iteration count, the byte model of one iteration
and its fraction of 8 TB/s, iterations and wall time to rtol; the same for FGMRES(30).  One JSON line per row."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import saddle_point_petsc_amd as S  # noqa: E402

PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=1024)
ap.add_argument("--its", type=int, default=300, help="iterations of the fixed-count runs (us per iteration)")
ap.add_argument("--rtol", type=float, default=1e-8)
ap.add_argument("--max-it", type=int, default=20000)
ap.add_argument("--minres-only", action="store_true", help="leave out the FGMRES rows (a short kernel trace)")
a = ap.parse_args()

A, f = S.AssembleOperator_Laplace(a.grid)
B, g = S.AssembleOperator_Constraints(a.grid)


def ctx(with_b, pc, fact):
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    if with_b:
        c.set_block(S.BLOCK_A10, B)
    c.pc_setup(pc, fact)
    return c


def minres_bytes(c, with_b, natural):
    """One iteration: the product (the A block in the layout it streams, B and B^T), the lagged update + <K z, z> pass
    (14 vector streams; 8 without the r / K w recurrences of the unpreconditioned norm) and the v / z pass (6: p, v_j,
    v_{j-1} in and v_{j+1} out, diag(A)^-1, z_{j+1})."""
    s = c.sizes()
    vec = 8 * (s["n_local"] + s["m"])
    prod = c.spmv_info()["layout_bytes"]
    if with_b:
        prod += 2 * 12 * B.nnz + 8 * s["n_local"]   # B^T lambda rows in the product epilogue, B z_0 (reads z_0 once more)
    streams = 20 - (6 if natural else 0)
    return prod + streams * vec, streams


rows = []
for name, with_b, pc, fact, fact_fg in (("saddle_diag", True, S.PC_SCHUR, S.SCHUR_DIAG, S.SCHUR_FULL),
                                         ("A_jacobi", False, S.PC_JACOBI, 0, 0)):
    rhs = np.concatenate([f, g]) if with_b else f
    c = ctx(with_b, pc, fact)
    c.minres(rhs, rtol=0.0, abstol=0.0, max_it=20)   # warm-up: first-use allocations
    for norm in ("unpreconditioned", "natural"):
        _, fixed = c.minres(rhs, norm=norm, rtol=0.0, abstol=0.0, max_it=a.its)
        us = fixed["solve_seconds"] / fixed["its"] * 1e6
        nbytes, streams = minres_bytes(c, with_b, norm == "natural")
        x, conv = c.minres(rhs, norm=norm, rtol=a.rtol, max_it=a.max_it)
        true = np.linalg.norm(rhs - c.mult(x)) / np.linalg.norm(rhs)
        rows.append(dict(system=name, grid=a.grid, solver="minres", norm=norm, us_per_it=round(us, 2),
                         model_bytes=nbytes, vector_streams=streams, tb_s=round(nbytes / us * 1e-6, 3),
                         frac_peak=round(nbytes / (us * 1e-6) / PEAK, 3), its=conv["its"], reason=conv["reason"],
                         cycles=conv["cycles"], seconds=round(conv["solve_seconds"], 4), true_rel_res=float(true)))
    c.close()
    if a.minres_only:
        continue
    c = ctx(with_b, pc, fact_fg)
    c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=30)
    _, fixed = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=a.its)
    x, conv = c.fgmres(rhs, rtol=a.rtol, max_it=a.max_it)
    true = np.linalg.norm(rhs - c.mult(x)) / np.linalg.norm(rhs)
    rows.append(dict(system=name, grid=a.grid, solver="fgmres", pc=("schur_full" if with_b else "jacobi"),
                     us_per_it=round(fixed["solve_seconds"] / fixed["its"] * 1e6, 2), its=conv["its"], reason=conv["reason"],
                     seconds=round(conv["solve_seconds"], 4), true_rel_res=float(true)))
    c.close()
for r in rows:
    print(json.dumps(r), flush=True)
