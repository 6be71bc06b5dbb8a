#!/usr/bin/env python3
"""Grid-coarsening multigrid (-pc_type mg) against the smoothed aggregation it leaves untouched (-pc_type gamg) on one
GPU, in one process:
    python tools/mg_bench.py [--grids 257 513 1025] [--sides odd|any] [--reps 5] [--out profiles/FILE.jsonl]
--sides any (-spk_mg_sides any) lets mg coarsen even sides, so --grids 256 512 1024 run; every emitted line records it.
K = A, FGMRES(30) to rtol 1e-8, both hierarchies built on the device.  Per grid one context per preconditioner; after one
warm-up round, --reps alternating rounds of set-up -> solve -> V-cycle timing (spk_pc_apply back to back on device
vectors).  Per row: levels, operator complexity, and median (min..max) of the V-cycle, the solve, the set-up and set-up +
solve, with the iterations.  The bar, checked at the largest grid: mg's solve median plus its spread (max - min) at or
below gamg's solve median; the exit status is 1 when it is missed.  Then the saddle system with Schur FULL and the exact
Schur complement (schur_pre="full"), the same comparison, reported only.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mg_bench.py --transfers [--grid 1025]
    python tools/mg_bench.py --transfers-report DIR [--grid 1025] [--out profiles/FILE.jsonl]
The two transfers of level 0 alone, through the test hook (one launch per call, on fresh copies of the same vectors):
after one warm-up round, --reps alternating rounds of the matrix-free prolongation, the stored one (amg_csr_kernel<3> on
P), the matrix-free restriction and the stored one (amg_csr_kernel<2> on R), all on the hierarchy of one context.  The
report reads the kernel trace of that run: median (min..max) per kernel, the fraction of the byte model
(prolongation: y read + y written + e read; restriction: b + t read + b_c written) at the HBM peak, and the bar --
matrix-free median plus its spread below the stored median -- with exit status 1 when it is missed.
    python tools/mg_bench.py --galerkin both [--grids 1025] [--sides odd|any] [--out profiles/FILE.jsonl]
--galerkin products|stencil (-spk_mg_galerkin; default products) selects what forms mg's coarse operators in the runs
above; every emitted line records it.  --galerkin both compares the two instead of mg and gamg: K = A, per grid two
contexts in one process, reuse off so that every set-up is a build, after one warm-up round --reps alternating rounds of
set-up -> solve -> V-cycle timing; then, per context, a reuse-on refresh on the values of a kappa-scaled operator.  Per
route: set-up, solve, iterations, V-cycle, refresh and nnz per level.  The bar, checked at 1025 and 1024 nodes per side:
the stencil route's set-up median plus its spread (max - min) at or below the products route's set-up median (exit
status 1 when missed); the iterations of the two must agree within 1.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mg_bench.py --setup-only stencil [--grid 1025]
--setup-only products|stencil launches builds alone (a warm-up and --reps more), for a kernel trace.
    python tools/mg_bench.py --operator both --galerkin stencil [--grids 1025] [--sides odd|any] [--out profiles/FILE.jsonl]
--operator csr|stencil (-spk_mg_operator; default csr) selects how mg's cycle applies the levels between level 0 and the
coarsest in the runs above (stencil needs --galerkin stencil); every emitted line records it.  --operator both compares
the two: K = A, per grid two contexts on the same hierarchy bytes in one process, after one warm-up round --reps
alternating rounds of set-up -> solve -> V-cycle timing.  Per route: V-cycle, solve, iterations and set-up.  The bar,
checked at 1025 and 1024 nodes per side: the stencil route's V-cycle median plus its spread (max - min) at or below the csr
route's V-cycle median (exit status 1 when missed); the iterations of the two must agree within 1.
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mg_bench.py --operator-kernels [--grid 1025]
    python tools/rocpd_by_grid.py DIR/<host>/<pid>_results.db out.csv amg_stencil_kernel amg_csr_kernel
--operator-kernels launches the product and the smoothing step of levels 1 and 2 alone through the test hook, on both
routes alternating (a warm-up round and --reps more), for a kernel trace; tools/rocpd_by_grid.py tells the levels apart by
their launch grids.  The line it prints has the byte models: 8 B per stored entry (csr: 12 B and the row pointers) plus
the vectors.
    python tools/mg_bench.py --lanczos both --galerkin stencil [--grids 1025] [--sides odd|any] [--out profiles/FILE.jsonl]
--lanczos stepwise|resident (-spk_amg_lanczos; default stepwise) selects who holds the scalars of the device set-up's
Lanczos in the runs above; every emitted line records it.  --lanczos both compares the two: K = A, per grid two contexts in
one process, reuse off so that every set-up is a build, after one warm-up round --reps alternating rounds of set-up -> solve
-> V-cycle timing; then, per context, reuse-on refreshes on alternating values.  Per route: set-up and refresh as median
(min..max) with the read-backs of the Ritz estimates, solve, iterations and V-cycle.  The bar, checked at 1025 and 1024
nodes per side, for the build and for the refresh: the resident route's median plus its spread (max - min) at or below the
stepwise route's median (exit status 1 when missed); iterations and lambda_max of the two must be equal.
    python tools/mg_bench.py --precision both --galerkin stencil --operator stencil [--grids 1025] [--sides odd|any] [--dim 2|3]
--precision double|single (-spk_mg_precision; default double) selects what the levels >= 1 of mg's cycle run in in the runs
above (single needs --galerkin stencil --operator stencil); every emitted line records it.  --precision both compares the
two: K = A, per grid two contexts on the same hierarchy bytes in one process, after one warm-up round --reps alternating
rounds of set-up -> solve -> V-cycle timing.  Per route: V-cycle, solve, iterations and set-up.  --dim 3: the 3-D generator
on a cube of --grids nodes per side (bs 3).  The bar, checked at 1025 and 1024 nodes per side: single's V-cycle median plus
its spread (max - min) at or below double's V-cycle median (exit status 1 when missed); the iterations of the two must
agree within 1.
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mg_bench.py --precision-kernels [--grid 1025]
    python tools/rocpd_by_grid.py DIR/<host>/<pid>_results.db out.csv amg_stencil_kernel amg_stencil_f32_kernel
--precision-kernels launches the product and the smoothing step of levels 1 and 2 alone through the two test hooks, FP64
and FP32 alternating (a warm-up round and --reps more), for a kernel trace; the line it prints has the byte models: 8 B
or 4 B per stored entry plus the vectors."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

PEAK = 8.0e12   # HBM bytes per second

ap = argparse.ArgumentParser()
ap.add_argument("--grids", type=int, nargs="+", default=[257, 513, 1025])
ap.add_argument("--grid", type=int, default=1025, help="--transfers / --transfers-report: nodes per side")
ap.add_argument("--sides", choices=["odd", "any"], default="odd", help="mg's side rule (-spk_mg_sides)")
ap.add_argument("--rtol", type=float, default=1e-8)
ap.add_argument("--reps", type=int, default=5, help="alternating rounds after the warm-up round")
ap.add_argument("--no-saddle", action="store_true", help="leave out the saddle rows")
ap.add_argument("--transfers", action="store_true", help="only launch the level-0 transfers (for a kernel trace)")
ap.add_argument("--transfers-report", metavar="DIR", help="read the kernel trace a --transfers run left under DIR")
ap.add_argument("--galerkin", choices=["products", "stencil", "both"], default="products", help="mg's coarse operators (-spk_mg_galerkin)")
ap.add_argument("--setup-only", choices=["products", "stencil"], help="only launch device builds of --grid (for a kernel trace)")
ap.add_argument("--operator", choices=["csr", "stencil", "both"], default="csr", help="how mg's cycle applies the levels >= 1 (-spk_mg_operator)")
ap.add_argument("--operator-kernels", action="store_true", help="only launch the level operators of levels 1 and 2 of --grid (for a kernel trace)")
ap.add_argument("--lanczos", choices=["stepwise", "resident", "both"], default="stepwise",
                help="who holds the scalars of the device set-up's Lanczos (-spk_amg_lanczos)")
ap.add_argument("--precision", choices=["double", "single", "both"], default="double", help="what mg's levels >= 1 run in (-spk_mg_precision)")
ap.add_argument("--precision-kernels", action="store_true", help="only launch the FP64 and FP32 level operators of levels 1 and 2 of --grid (for a kernel trace)")
ap.add_argument("--dim", type=int, choices=[2, 3], default=2, help="--precision both: the 2-D generator, or the 3-D one on a cube")
ap.add_argument("--out", help="append the JSON lines to this file too")
a = ap.parse_args()


def emit(row):
    line = json.dumps(dict(dict(galerkin=a.galerkin, operator=a.operator, lanczos=a.lanczos, precision=a.precision), **dict(row, sides=a.sides)))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def mmm(v, scale=1.0, digits=6):
    return dict(median=round(float(np.median(v)) * scale, digits), min=round(min(v) * scale, digits), max=round(max(v) * scale, digits))


def coarse_side(m):
    """the side rule: an odd side >= 5 halves, under `any` an even side >= 4 too, to m // 2 + 1"""
    return m // 2 + 1 if (m >= 4 if a.sides == "any" else m >= 5 and m % 2 == 1) else m


def transfer_models(grid):
    n, nc = 2 * grid * grid, 2 * coarse_side(grid) ** 2
    return dict(prolong=8 * (2 * n + nc), restrict=8 * (2 * n + nc))


if a.transfers_report:
    names = dict(prolong_matrixfree="amg_prolong_grid_kernel", restrict_matrixfree="amg_restrict_grid_kernel",
                 prolong_stored="amg_csr_kernel<3>", restrict_stored="amg_csr_kernel<2>")
    files = glob.glob(os.path.join(a.transfers_report, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {a.transfers_report}")
    rows = []
    for fn in files:
        with open(fn, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    model = transfer_models(a.grid)
    us = {}
    for key, sub in names.items():
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if sub in r["Kernel_Name"]]
        if len(d) < 2:
            sys.exit(f"{len(d)} launches of {sub} in the trace: run --transfers under the profiler first")
        us[key] = d[1:]   # the first launch of each is the warm-up round
    ok = True
    for what in ("prolong", "restrict"):
        mf, st = us[what + "_matrixfree"], us[what + "_stored"]
        met = float(np.median(mf)) + (max(mf) - min(mf)) < float(np.median(st))
        ok = ok and met
        emit(dict(mode="transfers", grid=a.grid, level=0, kernel=what, launches=len(mf), model_bytes=model[what],
                  matrixfree_us=mmm(mf, digits=2), stored_us=mmm(st, digits=2),
                  matrixfree_frac_peak=round(model[what] / (float(np.median(mf)) * 1e-6) / PEAK, 3),
                  stored_over_matrixfree=round(float(np.median(st) / np.median(mf)), 2),
                  bar="matrix-free median + spread < stored median", bar_met=bool(met)))
    sys.exit(0 if ok else 1)

import saddle_point_petsc_amd as S  # noqa: E402

if a.transfers:
    g = a.grid
    A, _ = S.AssembleOperator_Laplace(g, g)
    rng = np.random.default_rng(g)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(g, g), setup="device", sides=a.sides))
        info = c.amg_info()
        nf, nc = info["rows"][0], info["rows"][1]
        e, y, b, t = rng.standard_normal(nc), rng.standard_normal(nf), rng.standard_normal(nf), rng.standard_normal(nf)
        for rep in range(-1, a.reps):
            for stored in (False, True):
                c.debug_amg_transfer(0, "prolong", e, y, stored=stored)
            for stored in (False, True):
                c.debug_amg_transfer(0, "restrict", b, t, stored=stored)
    print(json.dumps(dict(mode="transfers-launched", grid=g, sides=a.sides, rows=[nf, nc], rounds=a.reps + 1)), flush=True)
    sys.exit(0)

if a.setup_only:
    g = a.grid
    A, _ = S.AssembleOperator_Laplace(g, g)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        for rep in range(-1, a.reps):
            c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(g, g), setup="device", sides=a.sides, galerkin=a.setup_only))
        info = c.amg_info()
    print(json.dumps(dict(mode="setup-only-launched", grid=g, sides=a.sides, galerkin=a.setup_only, builds=a.reps + 1, rows=info["rows"],
                          nnz=info["nnz"])), flush=True)
    sys.exit(0)


def mg_opts(g, galerkin, operator=None, lanczos=None, precision=None, dim=2):
    return dict(coarsening="grid", grid=(g, g) if dim == 2 else (g, g, g), setup="device", sides=a.sides, galerkin=galerkin,
                operator=operator or (a.operator if a.operator != "both" else "csr"),
                lanczos=lanczos or (a.lanczos if a.lanczos != "both" else "stepwise"),
                precision=precision or (a.precision if a.precision != "both" else "double"))


if a.precision_kernels:
    g = a.grid
    A, _ = S.AssembleOperator_Laplace(g, g)
    rng = np.random.default_rng(g)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, "stencil", "stencil", precision="single"))
        info = c.amg_info()
        models = []
        for l in (1, 2):
            n, nnz = info["rows"][l], info["nnz"][l]
            x, xo, b = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
            for rep in range(-1, a.reps):
                for prec in ("double", "single"):
                    c.debug_amg_operator(l, "product", x, precision=prec)
                    c.debug_amg_operator(l, "step", x, b=b, xo=xo, alpha=0.7, beta=0.3, precision=prec)
            # x read + out written; the step: + D^-1, b, y-
            models.append(dict(level=l, rows=n, nnz=nnz, dims=info["dims"][l],
                               double_product_bytes=8 * nnz + 16 * n, double_step_bytes=8 * nnz + 40 * n,
                               single_product_bytes=4 * nnz + 8 * n, single_step_bytes=4 * nnz + 20 * n))
    print(json.dumps(dict(mode="precision-kernels-launched", grid=g, sides=a.sides, rounds=a.reps + 1, levels=models)), flush=True)
    sys.exit(0)


if a.operator_kernels:
    g = a.grid
    A, _ = S.AssembleOperator_Laplace(g, g)
    rng = np.random.default_rng(g)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, "stencil", "stencil"))
        info = c.amg_info()
        models = []
        for l in (1, 2):
            n, nnz = info["rows"][l], info["nnz"][l]
            x, xo, b = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
            for rep in range(-1, a.reps):
                for stencil in (False, True):
                    c.debug_amg_operator(l, "product", x, stencil=stencil)
                    c.debug_amg_operator(l, "step", x, b=b, xo=xo, alpha=0.7, beta=0.3, stencil=stencil)
            # x read + out written; the step: + D^-1, b, y-
            models.append(dict(level=l, rows=n, nnz=nnz, dims=info["dims"][l],
                               stencil_product_bytes=8 * nnz + 16 * n, stencil_step_bytes=8 * nnz + 40 * n,
                               csr_product_bytes=12 * nnz + 4 * (n + 1) + 16 * n, csr_step_bytes=12 * nnz + 4 * (n + 1) + 40 * n))
    print(json.dumps(dict(mode="operator-kernels-launched", grid=g, sides=a.sides, rounds=a.reps + 1, levels=models)), flush=True)
    sys.exit(0)


def compare_galerkin(g):
    """the two routes of mg's coarse operators on K = A; returns {route: (set-up seconds, iterations)}"""
    A, f = S.AssembleOperator_Laplace(g, g)
    A1, _ = S.AssembleOperator_Laplace(g, g, kappa=1.0 + np.random.default_rng(g).random((g - 1) * (g - 1)))
    routes = ("products", "stencil")
    ctxs, t = {}, {}
    for route in routes:
        c = S.Context(0)
        c.set_block(S.BLOCK_A00, A)
        ctxs[route] = c
        t[route] = dict(setup=[], solve=[], vcycle=[], its=[], res=[], refresh=[])
    for rep in range(-1, a.reps):   # -1: the warm-up round, not counted; reuse off: every set-up builds
        for route, c in ctxs.items():
            c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, route))
            x, info = c.fgmres(f, rtol=a.rtol, max_it=500, restart=30)
            assert info["reason"] == 2, (route, info["reason"])
            vc_ms = c.time_kernel("pc", warmup=5, reps=50)
            if rep < 0:
                continue
            r = t[route]
            r["setup"].append(c.amg_info()["setup_seconds"])
            r["solve"].append(info["solve_seconds"])
            r["vcycle"].append(vc_ms * 1e-3)
            r["its"].append(info["its"])
            r["res"].append(float(np.linalg.norm(f - c.mult(x)) / np.linalg.norm(f)))
    infos = {route: c.amg_info() for route, c in ctxs.items()}
    for route, c in ctxs.items():   # reuse on: one build, then refreshes on alternating values of the same pattern
        c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, route), amg_reuse=True)
        for rep in range(-1, a.reps):
            c.set_block(S.BLOCK_A00, A1 if rep % 2 else A)
            c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, route), amg_reuse=True)
            ri = c.amg_reuse_info()
            assert ri["refreshed"], route
            if rep >= 0:
                t[route]["refresh"].append(ri["seconds"])
    for route, c in ctxs.items():
        info, r = infos[route], t[route]
        emit(dict(mode="galerkin", system="A", grid=g, pc="mg", route=route, solver="fgmres(30)", rtol=a.rtol, reps=a.reps,
                  levels=info["levels"], rows=info["rows"], nnz=info["nnz"], operator_complexity=round(info["operator_complexity"], 4),
                  its=sorted(set(r["its"])), true_rel_res=max(r["res"]), pc_apply_us=mmm(r["vcycle"], 1e6, 1),
                  solve_ms=mmm(r["solve"], 1e3, 3), setup_ms=mmm(r["setup"], 1e3, 3), refresh_ms=mmm(r["refresh"], 1e3, 3)))
        c.close()
    return {route: (t[route]["setup"], t[route]["its"]) for route in routes}


def compare_operator(g):
    """the two routes of the level operators on K = A over the same hierarchy; returns {route: (V-cycle seconds, iterations)}"""
    A, f = S.AssembleOperator_Laplace(g, g)
    routes = ("csr", "stencil")
    ctxs, t = {}, {}
    for route in routes:
        c = S.Context(0)
        c.set_block(S.BLOCK_A00, A)
        ctxs[route] = c
        t[route] = dict(setup=[], solve=[], vcycle=[], its=[], res=[])
    for rep in range(-1, a.reps):   # -1: the warm-up round, not counted
        for route, c in ctxs.items():
            c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, "stencil", route))
            x, info = c.fgmres(f, rtol=a.rtol, max_it=500, restart=30)
            assert info["reason"] == 2, (route, info["reason"])
            vc_ms = c.time_kernel("pc", warmup=5, reps=50)
            if rep < 0:
                continue
            r = t[route]
            r["setup"].append(c.amg_info()["setup_seconds"])
            r["solve"].append(info["solve_seconds"])
            r["vcycle"].append(vc_ms * 1e-3)
            r["its"].append(info["its"])
            r["res"].append(float(np.linalg.norm(f - c.mult(x)) / np.linalg.norm(f)))
    for route, c in ctxs.items():
        info, r = c.amg_info(), t[route]
        assert info["operator"] == (route == "stencil")
        emit(dict(mode="operator", system="A", grid=g, pc="mg", route=route, solver="fgmres(30)", rtol=a.rtol, reps=a.reps,
                  levels=info["levels"], rows=info["rows"], nnz=info["nnz"], operator_complexity=round(info["operator_complexity"], 4),
                  its=sorted(set(r["its"])), true_rel_res=max(r["res"]), pc_apply_us=mmm(r["vcycle"], 1e6, 1),
                  solve_ms=mmm(r["solve"], 1e3, 3), setup_ms=mmm(r["setup"], 1e3, 3)))
        c.close()
    return {route: (t[route]["vcycle"], t[route]["its"]) for route in routes}


def compare_precision(g):
    """FP64 and FP32 levels >= 1 on K = A over the same hierarchy; returns {route: (V-cycle seconds, iterations)}"""
    A, f = S.AssembleOperator_Laplace(g, g) if a.dim == 2 else S.AssembleOperator_Laplace3D(g, g, g)
    routes = ("double", "single")
    ctxs, t = {}, {}
    for route in routes:
        c = S.Context(0)
        c.set_block(S.BLOCK_A00, A)
        ctxs[route] = c
        t[route] = dict(setup=[], solve=[], vcycle=[], its=[], res=[])
    for rep in range(-1, a.reps):   # -1: the warm-up round, not counted
        for route, c in ctxs.items():
            c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, "stencil", "stencil", precision=route, dim=a.dim))
            x, info = c.fgmres(f, rtol=a.rtol, max_it=500, restart=30)
            assert info["reason"] == 2, (route, info["reason"])
            vc_ms = c.time_kernel("pc", warmup=5, reps=50)
            if rep < 0:
                continue
            r = t[route]
            r["setup"].append(c.amg_info()["setup_seconds"])
            r["solve"].append(info["solve_seconds"])
            r["vcycle"].append(vc_ms * 1e-3)
            r["its"].append(info["its"])
            r["res"].append(float(np.linalg.norm(f - c.mult(x)) / np.linalg.norm(f)))
    for route, c in ctxs.items():
        info, r = c.amg_info(), t[route]
        assert info["precision"] == (route == "single")
        emit(dict(mode="precision", system="A", dim=a.dim, grid=g, pc="mg", route=route, solver="fgmres(30)", rtol=a.rtol, reps=a.reps,
                  levels=info["levels"], rows=info["rows"], nnz=info["nnz"], operator_complexity=round(info["operator_complexity"], 4),
                  its=sorted(set(r["its"])), true_rel_res=max(r["res"]), pc_apply_us=mmm(r["vcycle"], 1e6, 1),
                  solve_ms=mmm(r["solve"], 1e3, 3), setup_ms=mmm(r["setup"], 1e3, 3)))
        c.close()
    return {route: (t[route]["vcycle"], t[route]["its"]) for route in routes}


def compare_lanczos(g):
    """the two routes of the set-up's Lanczos on K = A: the same hierarchy; returns {route: (set-up seconds, refresh seconds, its)}"""
    A, f = S.AssembleOperator_Laplace(g, g)
    A1, _ = S.AssembleOperator_Laplace(g, g, kappa=1.0 + np.random.default_rng(g).random((g - 1) * (g - 1)))
    routes = ("stepwise", "resident")
    galerkin = a.galerkin if a.galerkin != "both" else "stencil"
    ctxs, t = {}, {}
    for route in routes:
        c = S.Context(0)
        c.set_block(S.BLOCK_A00, A)
        ctxs[route] = c
        t[route] = dict(setup=[], solve=[], vcycle=[], its=[], res=[], refresh=[])
    for rep in range(-1, a.reps):   # -1: the warm-up round, not counted; reuse off: every set-up builds
        for route, c in ctxs.items():
            c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, galerkin, lanczos=route))
            x, info = c.fgmres(f, rtol=a.rtol, max_it=500, restart=30)
            assert info["reason"] == 2, (route, info["reason"])
            vc_ms = c.time_kernel("pc", warmup=5, reps=50)
            if rep < 0:
                continue
            r = t[route]
            r["setup"].append(c.amg_info()["setup_seconds"])
            r["solve"].append(info["solve_seconds"])
            r["vcycle"].append(vc_ms * 1e-3)
            r["its"].append(info["its"])
            r["res"].append(float(np.linalg.norm(f - c.mult(x)) / np.linalg.norm(f)))
    infos = {route: c.amg_info() for route, c in ctxs.items()}
    assert infos["stepwise"]["lambda_max"] == infos["resident"]["lambda_max"], "the two routes estimate different Ritz values"
    refresh_reads = {}
    for route, c in ctxs.items():   # reuse on: one build, then refreshes on alternating values of the same pattern
        c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, galerkin, lanczos=route), amg_reuse=True)
        for rep in range(-1, a.reps):
            c.set_block(S.BLOCK_A00, A1 if rep % 2 else A)
            c.pc_setup(S.PC_JACOBI, amg=mg_opts(g, galerkin, lanczos=route), amg_reuse=True)
            ri = c.amg_reuse_info()
            assert ri["refreshed"], route
            if rep >= 0:
                t[route]["refresh"].append(ri["seconds"])
        refresh_reads[route] = c.amg_info()["ritz_readbacks"]
    for route, c in ctxs.items():
        info, r = infos[route], t[route]
        assert info["lanczos"] == (route == "resident")
        emit(dict(mode="lanczos", system="A", grid=g, pc="mg", route=route, galerkin=galerkin, solver="fgmres(30)", rtol=a.rtol,
                  reps=a.reps, levels=info["levels"], rows=info["rows"], ritz_readbacks=info["ritz_readbacks"],
                  refresh_ritz_readbacks=refresh_reads[route], its=sorted(set(r["its"])), true_rel_res=max(r["res"]),
                  pc_apply_us=mmm(r["vcycle"], 1e6, 1), solve_ms=mmm(r["solve"], 1e3, 3), setup_ms=mmm(r["setup"], 1e3, 3),
                  refresh_ms=mmm(r["refresh"], 1e3, 3)))
        c.close()
    return {route: (t[route]["setup"], t[route]["refresh"], t[route]["its"]) for route in routes}


if a.precision == "both":
    if a.galerkin != "stencil" or a.operator != "stencil":
        sys.exit("--precision both compares two applications of the all-stencil route: pass --galerkin stencil --operator stencil")
    met = True
    for g in a.grids:
        s = compare_precision(g)
        (dv, di), (sv, si) = s["double"], s["single"]
        same_its = max(abs(u - v) for u in di for v in si) <= 1
        row = dict(mode="bar", system="A", dim=a.dim, grid=g, iterations_within_one=bool(same_its), double_pc_apply_us=mmm(dv, 1e6, 1),
                   single_pc_apply_us=mmm(sv, 1e6, 1), double_over_single=round(float(np.median(dv) / np.median(sv)), 3))
        met = met and same_its
        if a.dim == 2 and g in (1024, 1025):
            ok = float(np.median(sv)) + (max(sv) - min(sv)) <= float(np.median(dv))
            met = met and ok
            row.update(bar="single V-cycle median + spread <= double V-cycle median", bar_met=bool(ok))
        emit(row)
    sys.exit(0 if met else 1)

if a.lanczos == "both":
    met = True
    for g in a.grids:
        s = compare_lanczos(g)
        (ss, sr, si), (rs, rr, ri) = s["stepwise"], s["resident"]
        same_its = set(si) == set(ri)
        row = dict(mode="bar", system="A", grid=g, iterations_equal=bool(same_its), stepwise_setup_ms=mmm(ss, 1e3, 3),
                   resident_setup_ms=mmm(rs, 1e3, 3), stepwise_refresh_ms=mmm(sr, 1e3, 3), resident_refresh_ms=mmm(rr, 1e3, 3),
                   setup_stepwise_over_resident=round(float(np.median(ss) / np.median(rs)), 3),
                   refresh_stepwise_over_resident=round(float(np.median(sr) / np.median(rr)), 3))
        met = met and same_its
        if g in (1024, 1025):
            ok_b = float(np.median(rs)) + (max(rs) - min(rs)) <= float(np.median(ss))
            ok_r = float(np.median(rr)) + (max(rr) - min(rr)) <= float(np.median(sr))
            met = met and ok_b and ok_r
            row.update(bar="resident median + spread <= stepwise median, build and refresh", bar_met_build=bool(ok_b),
                       bar_met_refresh=bool(ok_r))
        emit(row)
    sys.exit(0 if met else 1)

if a.operator == "both":
    if a.galerkin != "stencil":
        sys.exit("--operator both compares two applications of stencil-built levels: pass --galerkin stencil")
    met = True
    for g in a.grids:
        s = compare_operator(g)
        (cv, ci), (sv, si) = s["csr"], s["stencil"]
        same_its = max(abs(u - v) for u in ci for v in si) <= 1
        row = dict(mode="bar", system="A", grid=g, iterations_within_one=bool(same_its), csr_pc_apply_us=mmm(cv, 1e6, 1),
                   stencil_pc_apply_us=mmm(sv, 1e6, 1), csr_over_stencil=round(float(np.median(cv) / np.median(sv)), 3))
        met = met and same_its
        if g in (1024, 1025):
            ok = float(np.median(sv)) + (max(sv) - min(sv)) <= float(np.median(cv))
            met = met and ok
            row.update(bar="stencil V-cycle median + spread <= csr V-cycle median", bar_met=bool(ok))
        emit(row)
    sys.exit(0 if met else 1)

if a.galerkin == "both":
    met = True
    for g in a.grids:
        s = compare_galerkin(g)
        (ps, pi), (ss, si) = s["products"], s["stencil"]
        same_its = max(abs(u - v) for u in pi for v in si) <= 1
        row = dict(mode="bar", system="A", grid=g, iterations_within_one=bool(same_its), products_setup_ms=mmm(ps, 1e3, 3),
                   stencil_setup_ms=mmm(ss, 1e3, 3), products_over_stencil=round(float(np.median(ps) / np.median(ss)), 2))
        met = met and same_its
        if g in (1024, 1025):
            ok = float(np.median(ss)) + (max(ss) - min(ss)) <= float(np.median(ps))
            met = met and ok
            row.update(bar="stencil set-up median + spread <= products set-up median", bar_met=bool(ok))
        emit(row)
    sys.exit(0 if met else 1)

KINDS = dict(mg=lambda g: mg_opts(g, a.galerkin), gamg=lambda g: dict(setup="device"))


def compare(system, g, A, B, rhs):
    """one context per preconditioner, alternating rounds; returns {kind: solve seconds}"""
    pc, pre = (S.PC_JACOBI, "selfp") if B is None else (S.PC_SCHUR, "full")
    ctxs, t = {}, {}
    for kind in KINDS:
        c = S.Context(0)
        c.set_block(S.BLOCK_A00, A)
        if B is not None:
            c.set_block(S.BLOCK_A10, B)
        ctxs[kind] = c
        t[kind] = dict(setup=[], solve=[], vcycle=[], its=[], res=[])
    for rep in range(-1, a.reps):   # -1: the warm-up round, not counted
        for kind, c in ctxs.items():
            c.pc_setup(pc, S.SCHUR_FULL, amg=KINDS[kind](g), schur_pre=pre)
            x, info = c.fgmres(rhs, rtol=a.rtol, max_it=500, restart=30)
            assert info["reason"] == 2, (kind, info["reason"])
            vc_ms = c.time_kernel("pc", warmup=5, reps=50)
            if rep < 0:
                continue
            r = t[kind]
            r["setup"].append(c.amg_info()["setup_seconds"])
            r["solve"].append(info["solve_seconds"])
            r["vcycle"].append(vc_ms * 1e-3)
            r["its"].append(info["its"])
            r["res"].append(float(np.linalg.norm(rhs - c.mult(x)) / np.linalg.norm(rhs)))
    for kind, c in ctxs.items():
        info, r = c.amg_info(), t[kind]
        emit(dict(mode="solve", system=system, grid=g, pc=kind, solver="fgmres(30)", rtol=a.rtol, reps=a.reps, levels=info["levels"],
                  rows=info["rows"], operator_complexity=round(info["operator_complexity"], 4), its=sorted(set(r["its"])),
                  true_rel_res=max(r["res"]), pc_apply_us=mmm(r["vcycle"], 1e6, 1), solve_ms=mmm(r["solve"], 1e3, 3),
                  setup_ms=mmm(r["setup"], 1e3, 3),
                  setup_plus_solve_ms=mmm([u + v for u, v in zip(r["setup"], r["solve"])], 1e3, 3)))
        c.close()
    return {kind: t[kind]["solve"] for kind in KINDS}


met = True
for g in a.grids:
    A, f = S.AssembleOperator_Laplace(g, g)
    s = compare("A", g, A, None, f)
    if g == max(a.grids):
        mg, gamg = s["mg"], s["gamg"]
        met = float(np.median(mg)) + (max(mg) - min(mg)) <= float(np.median(gamg))
        emit(dict(mode="bar", system="A", grid=g, bar="mg solve median + spread <= gamg solve median",
                  mg_solve_ms=mmm(mg, 1e3, 3), gamg_solve_ms=mmm(gamg, 1e3, 3), bar_met=bool(met)))
    if not a.no_saddle:
        B, gg = S.AssembleOperator_Constraints(g, g)
        compare("saddle_full_exact_schur", g, A, B, np.concatenate([f, gg]))
sys.exit(0 if met else 1)
