#!/usr/bin/env python3
"""The smoothed-aggregation multigrid preconditioner (-pc_type gamg) against Jacobi FGMRES and MINRES on one GPU, in
one process:
    python tools/gamg_bench.py [--grids 256 512 1024] [--rtol 1e-8] [--max-it 20000]
Two systems: K = A (gamg in Jacobi's slot; FGMRES + Jacobi; MINRES + Jacobi) and the saddle system with Schur FULL
(-fieldsplit_0_pc_type gamg; FGMRES + the plain Schur FULL; MINRES + Schur DIAG).  Per gamg row: set-up time of both
routes (host build + upload, and -spk_gamg_setup device; each after one warm-up build, in this process) with the
iterations and time of the solve on the device-built hierarchy, levels, rows and operator complexity, the V-cycle's time (spk_pc_apply on device vectors, back to back) against its
byte model per level, iterations and wall time to rtol.  One JSON line per row.
    python tools/gamg_bench.py --schur-full [--reps 3]
The saddle system with FULL + gamg under both Schur preconditions, from one context per grid: after one warm-up set-up and
solve of each, --reps alternating rounds of selfp (S^ = diag(B diag(A)^-1 B^T), today's rows) and full (the exact dense
S = B V B^T, schur_pre="full").  Per row: iterations and solve time to rtol, the true residual, microseconds per PCApply
(back to back on device vectors), what W and S added to the set-up, and K = A's iteration count on the same grid.
    python tools/gamg_bench.py --refresh [--setup-only host|device|both] [--reps 5] [--out profiles/FILE.jsonl]
The refresh of the hierarchy (amg_reuse=True, -pc_gamg_reuse_interpolation) against a full build in the same process on
the same values, K = A, per grid and route on one context: one warm-up build, then --reps rounds of
  full build on the new values with reuse off (what every set-up did before the option) -> solve,
  build on the old values with reuse on (not compared: it only leaves a hierarchy to refresh) ,
  refresh to the new values -> solve.
The new values are the old ones scaled by s[row] s[col], s = 1 + 0.5 sin(2 pi i / n) cos(3 pi j / n) per node.  Per row:
median, minimum and maximum of the set-up seconds (spk_get_amg_reuse_info: the hierarchy alone, up to a device
synchronise) and of the whole pc_setup, and iterations and time of the solves to rtol.  --setup-only leaves the solves
out and names the routes (a kernel trace of build and refresh alone); --out appends the lines to a file as well."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import saddle_point_petsc_amd as S  # noqa: E402

PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--grids", type=int, nargs="+", default=[256, 512, 1024])
ap.add_argument("--rtol", type=float, default=1e-8)
ap.add_argument("--max-it", type=int, default=20000)
ap.add_argument("--gamg-only", action="store_true", help="leave out the Jacobi / MINRES rows (a short kernel trace)")
ap.add_argument("--setup-only", choices=["host", "device", "both"], help="only build the K = A hierarchy (after one "
                "warm-up build of each route asked for) and print one line per grid: a kernel trace of the set-up alone")
ap.add_argument("--schur-full", action="store_true", help="only the saddle rows of FULL + gamg, selfp and the exact Schur "
                "complement alternating in one process")
ap.add_argument("--reps", type=int, default=None, help="alternating rounds after the warm-up round (--schur-full: 3, --refresh: 5)")
ap.add_argument("--refresh", action="store_true", help="only the refresh of the K = A hierarchy against a full build on the "
                "same values, both routes (or those of --setup-only, then without the solves)")
ap.add_argument("--out", help="--refresh: append the JSON lines to this file too")
a = ap.parse_args()
if a.reps is None:
    a.reps = 5 if a.refresh else 3


def csr_bytes(nnz, n):
    return 12 * nnz + 4 * (n + 1)


def vcycle_model(c, info, nu):
    """Bytes one V-cycle moves, per level, for Chebyshev smoothing (beta_0 = 0, beta_k != 0 after: the step reads y-).
    A step from the zero guess (the first pre-smoothing step) moves dinv, b and out.  Level 0 on the 2x2 row-type
    layout: the fused step streams the layout (spmv_info: codes + y gathered + out written) and dinv, b (, y-); other
    layouts: the layout's product, then a pass over dinv, b, t, y (, y-), out.  Levels >= 1: CSR (12 B per entry + row
    pointers), the fused step reads x, dinv, b (, y-) and writes out.  Per level besides: the residual product, the
    restriction R (b - t) (R, b, t, the coarse b), the prolongation y += P e (P, y read and written, e); level 0 the
    output copy; the coarsest level the dense inverse."""
    L = info["levels"]
    betas = [0] + [1] * (nu - 1)
    steps_from_y = betas[1:] + betas   # pre-smoothing after its zero-guess step, then all of post-smoothing
    fused0 = c.spmv_info()["format"] == "dict2x2"
    per = []
    for l in range(L):
        n = info["rows"][l]
        v = 8 * n
        if l == L - 1:
            per.append(8 * n * n + 2 * v)
            continue
        rp, ci, _, shp = c.amg_level(l, S.AMG_PROLONG)
        pnnz, nc = len(ci), shp[1]
        if l == 0:
            prod = c.spmv_info()["layout_bytes"]
            step = (lambda be: prod + 2 * v + be * v) if fused0 else (lambda be: prod + 5 * v + be * v)
            res = prod
        else:
            prod = csr_bytes(info["nnz"][l], n)
            step = lambda be: prod + 4 * v + be * v
            res = prod + 2 * v
        steps = 3 * v + sum(step(be) for be in steps_from_y)
        restrict = csr_bytes(pnnz, nc) + 2 * v + 8 * nc
        prolong = csr_bytes(pnnz, n) + 2 * v + 8 * nc
        per.append(steps + res + restrict + prolong + (2 * v if l == 0 else 0))
    fine_step = (c.spmv_info()["layout_bytes"] + 3 * 8 * info["rows"][0]) if fused0 else None
    return per, fine_step


def ctx(A, B, pc, fact, amg=None):
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    if B is not None:
        c.set_block(S.BLOCK_A10, B)
    t0 = time.perf_counter()
    c.pc_setup(pc, fact, amg=amg)
    return c, time.perf_counter() - t0


def solve(c, rhs, solver, **kw):
    fn = c.fgmres if solver == "fgmres" else c.minres
    fn(rhs, rtol=0.0, abstol=0.0, max_it=5)   # first-use allocations
    x, info = fn(rhs, rtol=a.rtol, max_it=a.max_it, **kw)
    true = np.linalg.norm(rhs - c.mult(x)) / np.linalg.norm(rhs)
    return dict(its=info["its"], reason=info["reason"], seconds=round(info["solve_seconds"], 4), true_rel_res=float(true))


def setup_times(A, Bk, pc, fact, routes=("host", "device")):
    """set-up seconds of each route on one context (spk_amg_info.setup_seconds), after one warm-up build of each"""
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    if Bk is not None:
        c.set_block(S.BLOCK_A10, Bk)
    t = {}
    for rep in range(2):
        for route in routes:
            c.pc_setup(pc, fact, amg=dict(setup=route))
            t[route] = c.amg_info()["setup_seconds"]
    c.close()
    return t


def schur_full_rows(grid, A, f):
    B, g = S.AssembleOperator_Constraints(grid)
    rhs = np.concatenate([f, g])
    c, _ = ctx(A, None, S.PC_JACOBI, 0, amg=True)
    ka = solve(c, f, "fgmres")
    c.close()
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    c.set_block(S.BLOCK_A10, B)
    for rep in range(-1, a.reps):   # -1: the warm-up round (first-use allocations of either mode), not printed
        for pre in ("selfp", "full"):
            t0 = time.perf_counter()
            c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL, amg=True, schur_pre=pre)
            setup_wall = time.perf_counter() - t0
            conv = solve(c, rhs, "fgmres")
            pc_ms = c.time_kernel("pc", warmup=5, reps=50)
            if rep < 0:
                continue
            print(json.dumps(dict(system="saddle_full", grid=grid, solver="fgmres", pc="gamg", schur_pre=pre, rep=rep,
                                  setup_seconds=round(setup_wall, 4), schur_setup_seconds=round(c.schur_setup_seconds(), 6),
                                  pc_apply_us=round(pc_ms * 1e3, 1), ka_its=ka["its"], ka_seconds=ka["seconds"], **conv)),
                  flush=True)
    c.close()


def refresh_rows(grid, A, f):
    node = np.arange(A.nrows) // 2
    s = 1.0 + 0.5 * np.sin(2.0 * np.pi * (node % grid) / grid) * np.cos(3.0 * np.pi * (node // grid) / grid)
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    Anew = S.CSR(A.rowptr, A.colidx, A.val * s[rows] * s[A.colidx], A.nrows)
    routes = ("host", "device") if a.setup_only in (None, "both") else (a.setup_only,)
    for route in routes:
        c = S.Context(0)
        t = dict(build=[], refresh=[], build_pc_setup=[], refresh_pc_setup=[], build_solve=[], refresh_solve=[])
        its = dict(build=[], refresh=[])

        def setup(M, reuse, key=None):
            c.set_block(S.BLOCK_A00, M)
            t0 = time.perf_counter()
            c.pc_setup(S.PC_JACOBI, 0, amg=dict(setup=route), amg_reuse=reuse)
            wall = time.perf_counter() - t0
            r = c.amg_reuse_info()
            if key:
                assert r["refreshed"] == (key == "refresh"), (key, r)
                t[key].append(r["seconds"])
                t[key + "_pc_setup"].append(wall)
                if not a.setup_only:
                    conv = solve(c, f, "fgmres")
                    assert conv["reason"] == 2, conv
                    its[key].append(conv["its"])
                    t[key + "_solve"].append(conv["seconds"])

        setup(A, False)                       # warm-up build
        for _ in range(a.reps):
            setup(Anew, False, "build")       # the full build on the new values
            setup(A, True)                    # a hierarchy to refresh
            setup(Anew, True, "refresh")      # the refresh to the new values
        info = c.amg_info()
        c.close()
        row = dict(mode="refresh", system="A", grid=grid, route=route, reps=a.reps, levels=info["levels"])
        for key, v in t.items():
            if v:
                row[key + "_seconds"] = dict(median=round(float(np.median(v)), 5), min=round(min(v), 5), max=round(max(v), 5))
        row["build_over_refresh"] = round(float(np.median(t["build"]) / np.median(t["refresh"])), 2)
        for key, v in its.items():
            if v:
                row[key + "_its"] = sorted(set(v))
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


for grid in a.grids:
    A, f = S.AssembleOperator_Laplace(grid)
    if a.refresh:
        refresh_rows(grid, A, f)
        continue
    if a.schur_full:
        schur_full_rows(grid, A, f)
        continue
    if a.setup_only:
        routes = ("host", "device") if a.setup_only == "both" else (a.setup_only,)
        t = setup_times(A, None, S.PC_JACOBI, 0, routes)
        print(json.dumps(dict(system="A", grid=grid, **{r + "_setup_seconds": round(v, 4) for r, v in t.items()})), flush=True)
        continue
    B, g = S.AssembleOperator_Constraints(grid)
    for system, Bk, rhs, pc, fact, fact_mr in (("A", None, f, S.PC_JACOBI, 0, 0),
                                               ("saddle_full", B, np.concatenate([f, g]), S.PC_SCHUR, S.SCHUR_FULL,
                                                S.SCHUR_DIAG)):
        c, setup_wall = ctx(A, Bk, pc, fact, amg=True)
        info = c.amg_info()
        vc_ms = c.time_kernel("pc", warmup=5, reps=50)
        c.pc_setup(S.PC_JACOBI, 0, amg=True)   # the V-cycle alone (K = A slot) for the per-level model and timing
        vc_only_ms = c.time_kernel("pc", warmup=5, reps=50)
        model, fine_step = vcycle_model(c, info, 2)
        c.close()
        c, _ = ctx(A, Bk, pc, fact, amg=True)
        conv = solve(c, rhs, "fgmres")
        c.close()
        routes = setup_times(A, Bk, pc, fact)
        c, _ = ctx(A, Bk, pc, fact, amg=dict(setup="device"))
        dconv = solve(c, rhs, "fgmres")
        c.close()
        tot = sum(model)
        print(json.dumps(dict(system=system, grid=grid, solver="fgmres", pc="gamg", setup_seconds=round(setup_wall, 3),
                              host_setup_seconds=round(info["setup_seconds"], 3),
                              host_setup_warm_seconds=round(routes["host"], 4),
                              device_setup_warm_seconds=round(routes["device"], 4),
                              device_setup_its=dconv["its"], device_setup_solve_seconds=dconv["seconds"],
                              levels=info["levels"],
                              rows=info["rows"], operator_complexity=round(info["operator_complexity"], 4),
                              lambda_max=[round(x, 4) for x in info["lambda_max"]], pc_apply_us=round(vc_ms * 1e3, 1),
                              vcycle_us=round(vc_only_ms * 1e3, 1), vcycle_model_bytes=tot, vcycle_model_per_level=model,
                              vcycle_frac_peak=round(tot / (vc_only_ms * 1e-3) / PEAK, 3),
                              fine_step_model_bytes=fine_step, **conv)), flush=True)
        if a.gamg_only:
            continue
        c, _ = ctx(A, Bk, pc, fact)
        print(json.dumps(dict(system=system, grid=grid, solver="fgmres", pc="jacobi" if Bk is None else "schur_full",
                              **solve(c, rhs, "fgmres"))), flush=True)
        c.close()
        c, _ = ctx(A, Bk, pc, fact_mr)
        print(json.dumps(dict(system=system, grid=grid, solver="minres", pc="jacobi" if Bk is None else "schur_diag",
                              **solve(c, rhs, "minres"))), flush=True)
        c.close()
