#!/usr/bin/env python3
"""The fused coarse tail (-spk_mg_tail fused) and the W-cycle (-spk_mg_cycle w) against the V-cycle of launches, on one
GPU, in one process:
    python tools/mg_tail_bench.py [--grids 256 512 1024 257 513 1025] [--reps 5] [--cap 10000] [--out profiles/FILE.jsonl]
K = A.  Per grid: mg (an even side: with -spk_mg_sides any) and, on the even grids, gamg; one context per hierarchy,
built on the device with reuse on, so that a change of cycle / tail / tail_rows alone is a refresh.  After one warm-up of
every variant, --reps alternating rounds; per variant the median and min..max of
  - one application of the cycle back to back (spk_pc_apply on device vectors, device-synchronised),
  - FGMRES(30) to rtol 1e-8: iterations and solve time (V launches, V fused at the default tail_rows, every W variant),
and the launches of one application, counted from the step list (level 0 in the row-type layout: one launch per smoothing
step; one for the copy-out).  The variants: V with launches; V fused per tail_rows taken from the level sizes up to --cap
(the sweep behind SPK_AMG_TAIL_ROWS_DEFAULT; beats_launches: fused median + spread below the launches' median); W fused at
the default and per level size up to 1024; W with launches at 257 only (the record behind AUTO's choice under W).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mg_tail_bench.py --trace [--grid 1024]
    python tools/mg_tail_bench.py --trace-report DIR [--out profiles/FILE.jsonl]
The tail kernel's own time: --trace applies the fused V-cycle of mg and of gamg at one grid, the report reads the kernel
trace of that run."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grids", type=int, nargs="+", default=[256, 512, 1024, 257, 513, 1025])
ap.add_argument("--grid", type=int, default=1024, help="--trace: nodes per side")
ap.add_argument("--rtol", type=float, default=1e-8)
ap.add_argument("--reps", type=int, default=5, help="alternating rounds after the warm-up round")
ap.add_argument("--cap", type=int, default=10000, help="the largest level size the sweep takes as tail_rows")
ap.add_argument("--trace", action="store_true", help="only apply the fused V-cycle (for a kernel trace)")
ap.add_argument("--trace-report", metavar="DIR", help="read the kernel trace a --trace run left under DIR")
ap.add_argument("--out", help="append the JSON lines to this file too")
a = ap.parse_args()


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def mmm(v, scale=1.0, digits=6):
    return dict(median=round(float(np.median(v)) * scale, digits), min=round(min(v) * scale, digits), max=round(max(v) * scale, digits))


if a.trace_report:
    files = glob.glob(os.path.join(a.trace_report, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {a.trace_report}")
    rows = []
    for fn in files:
        with open(fn, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "amg_tail_kernel" in r["Kernel_Name"]]
    if len(d) < 4:
        sys.exit(f"{len(d)} launches of amg_tail_kernel in the trace: run --trace under the profiler first")
    half = len(d) // 2   # mg first, then gamg; the first launch of each is the warm-up
    emit(dict(mode="tail-kernel-trace", grid=a.grid, mg_tail_us=mmm(d[1:half], digits=2), gamg_tail_us=mmm(d[half + 1:], digits=2),
              launches=len(d)))
    sys.exit(0)

import saddle_point_petsc_amd as S  # noqa: E402


def kinds(g):
    out = {"mg": dict(coarsening="grid", grid=(g, g), setup="device", sides="odd" if g % 2 else "any")}
    if g % 2 == 0:
        out["gamg"] = dict(setup="device")
    return out


def count_launches(levels, cycle, tail_first, nu):
    n, s, steps = 1, 0, S.amg_cycle_steps(levels, cycle)   # 1: the copy-out
    while s < len(steps):
        kind, l = steps[s]
        if tail_first >= 1 and l >= tail_first:
            while s < len(steps) and steps[s][1] >= tail_first:
                s += 1
            n += 1
            continue
        n += nu if kind in (S.AMG_STEP_PRE0, S.AMG_STEP_PRE, S.AMG_STEP_POST) else 2 if kind == S.AMG_STEP_DOWN else 1
        s += 1
    return n


if a.trace:
    g = a.grid
    A, _ = S.AssembleOperator_Laplace(g, g)
    for kind, base in kinds(g).items():
        with S.Context(0) as c:
            c.set_block(S.BLOCK_A00, A)
            c.pc_setup(S.PC_JACOBI, amg=dict(base, cycle="v", tail="fused"))
            info = c.amg_info()
            c.time_kernel("pc", warmup=1, reps=20)
        print(json.dumps(dict(mode="trace-launched", grid=g, pc=kind, rows=info["rows"], tail_first=info["tail_first"])), flush=True)
    sys.exit(0)

for g in a.grids:
    A, f = S.AssembleOperator_Laplace(g, g)
    solves = {}
    for kind, base in kinds(g).items():
        with S.Context(0) as c:
            c.set_block(S.BLOCK_A00, A)
            c.pc_setup(S.PC_JACOBI, amg=base, amg_reuse=True)
            info = c.amg_info()
            rows, L, nu = info["rows"], info["levels"], 2
            variants = {"v_launches": dict(cycle="v", tail="launches")}
            for tr in sorted({r for r in rows[1:] if r <= a.cap}):
                variants[f"v_fused_{tr}"] = dict(cycle="v", tail="fused", tail_rows=tr)
            variants["v_fused_default"] = dict(cycle="v", tail="fused")
            for tr in sorted({r for r in rows[1:] if r <= 1024}):
                variants[f"w_fused_{tr}"] = dict(cycle="w", tail_rows=tr)
            variants["w_fused"] = dict(cycle="w")
            if g == 257:
                variants["w_launches"] = dict(cycle="w", tail="launches")
            solved = ["v_launches", "v_fused_default"] + [v for v in variants if v.startswith("w_")]
            t = {v: dict(apply=[], solve=[], its=[], res=[]) for v in variants}
            meta = {}
            for rep in range(-1, a.reps):   # -1: the warm-up round, not counted
                for v, kw in variants.items():
                    c.pc_setup(S.PC_JACOBI, amg=dict(base, **kw), amg_reuse=True)
                    assert c.amg_reuse_info()["refreshed"] is True
                    vi = c.amg_info()
                    meta[v] = dict(tail_first=vi["tail_first"], tail_launches=vi["tail_launches"],
                                   launches=count_launches(L, vi["cycle"], vi["tail_first"], nu))
                    ms = c.time_kernel("pc", warmup=3, reps=20 if v == "w_launches" else 50)
                    if v in solved:
                        x, si = c.fgmres(f, rtol=a.rtol, max_it=500, restart=30)
                        assert si["reason"] == 2, (kind, v, si["reason"])
                    if rep < 0:
                        continue
                    t[v]["apply"].append(ms * 1e-3)
                    if v in solved:
                        t[v]["solve"].append(si["solve_seconds"])
                        t[v]["its"].append(si["its"])
                        t[v]["res"].append(float(np.linalg.norm(f - c.mult(x)) / np.linalg.norm(f)))
            base_med = float(np.median(t["v_launches"]["apply"]))
            for v in variants:
                r = t[v]
                row = dict(mode="cycle", grid=g, pc=kind, variant=v, levels=L, rows=rows, reps=a.reps, **meta[v],
                           apply_us=mmm(r["apply"], 1e6, 1))
                if v.startswith("v_fused"):
                    row["beats_launches"] = bool(float(np.median(r["apply"])) + (max(r["apply"]) - min(r["apply"])) < base_med)
                if v in solved:
                    row.update(solver="fgmres(30)", rtol=a.rtol, its=sorted(set(r["its"])), true_rel_res=max(r["res"]),
                               solve_ms=mmm(r["solve"], 1e3, 3))
                    solves[kind, v] = float(np.median(r["solve"]))
                emit(row)
    if ("gamg", "v_launches") in solves:
        emit(dict(mode="mg-against-gamg", grid=g, **{f"{k}_{v}_solve_ms": round(s * 1e3, 3) for (k, v), s in solves.items()},
                  mg_fused_beats_gamg=bool(solves["mg", "v_fused_default"] < solves["gamg", "v_launches"]),
                  mg_launches_beats_gamg=bool(solves["mg", "v_launches"] < solves["gamg", "v_launches"])))
