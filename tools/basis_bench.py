#!/usr/bin/env python3
"""FP64 against FP32 storage of the FGMRES basis (-spk_basis_precision) on the headline workload: the saddle system with
the full Schur fieldsplit, FGMRES(30), whole restart cycles.

  python tools/basis_bench.py [--grid 1024] [--cycles 3] [--rounds 5] [--converge-grid 512] [--no-trace]
                              [--out profiles/basis_fp32_1024.jsonl]

Three configurations alternate in ONE process and on one context, `--rounds` times after one warm-up each:
  auto    FP64 basis, iteration_form 0 (what the library takes by default: form 7 on this shape)
  form5   FP64 basis, iteration_form 5 (the three-launch form the FP32 basis runs in)
  single  FP32 basis (form 5)
Every solve runs --cycles x 30 iterations (rtol far below reach, -ksp_max_it at a cycle's end); the figure is the solve's
own wall time (spk_result.solve_seconds: enqueue to the final synchronise, upload excluded) over its iterations.  The bar
-- single's median plus its min-to-max spread below auto's median -- is reported, not asserted.

The byte model counts FP64 vectors moved per iteration at the mean j of a cycle (form 5: the product's A stream + 3, MDot
j + 2 + p, kernel B j + 6 + p, p planes of B D): the FP32 basis halves the 2 (j + 1) basis reads and adds the newest
vector's second read in MDot.

Unless --no-trace, the tool then starts ONE child of itself under `rocprofv3 --kernel-trace --stats` (a form-5 and a
single solve) and reads the mean time of the two Gram-Schmidt kernels of either basis from its statistics; the rates are
those kernels' own bytes at the mean j over that time.  At last the iterations and the time to rtol 1e-8 on
--converge-grid."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import saddle_point_petsc_amd as S  # noqa: E402

RESTART = 30
CONFIGS = {"auto": dict(), "form5": dict(iteration_form=5), "single": dict(basis="single")}


def stat(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def context(grid):
    A, f = S.AssembleOperator_Laplace(grid)
    B, g = S.AssembleOperator_Constraints(grid)
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    c.set_block(S.BLOCK_A10, B)
    c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL)
    return c, np.concatenate([f, g]), A.nrows, B.nrows


def cycles_solve(c, rhs, cycles, **kw):
    _, info = c.fgmres(rhs, restart=RESTART, max_it=cycles * RESTART, rtol=1e-30, **kw)
    assert info["its"] == cycles * RESTART, info
    return info["solve_seconds"] / info["its"] * 1e6


def byte_model(c, n, m):
    """FP64 vectors per iteration at the mean j of a 30-cycle, form 5"""
    j = (RESTART - 1) / 2
    p = m / 2   # parity planes
    a_stream = c.spmv_info()["layout_bytes"] / (8.0 * n)
    double = a_stream + 3 + (j + 2 + p) + (j + 6 + p)
    single = double - (j + 1) + 0.5
    return dict(mean_j=j, planes=p, a_stream_vectors=round(a_stream, 2), fp64_vectors=round(double, 2), single_vectors=round(single, 2),
                expected_change=round(single / double - 1.0, 4))


def kernel_bytes(n, m):
    """own bytes of the two FP32-basis kernels and of their FP64 twins at the mean j"""
    j = (RESTART - 1) / 2
    planes = 8.0 * n * (m / 2)
    return {"mdot_f32_kernel": (j + 1) * 4 * n + 4 * n + 8 * n + planes,
            "iter_maxpy_uhead_kernel_f32": (j + 1) * 4 * n + 8 * n + 8 * n + planes + 4 * n + 8 * n + 8 * n,
            "mdot_kernel": (j + 1) * 8 * n + 8 * n + planes,
            "iter_maxpy_uhead_kernel_f64": (j + 1) * 8 * n + 8 * n + 8 * n + planes + 8 * n + 8 * n + 8 * n}


def trace_child(grid, cycles):
    c, rhs, _, _ = context(grid)
    for name in ("form5", "single"):
        cycles_solve(c, rhs, 1, **CONFIGS[name])
        cycles_solve(c, rhs, cycles, **CONFIGS[name])
    c.close()


def trace(grid, cycles, n, m):
    exe = shutil.which("rocprofv3")
    if not exe:
        return dict(skipped="rocprofv3 not found")
    d = tempfile.mkdtemp(prefix="basis_trace_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--trace-child", "--grid", str(grid), "--cycles", str(cycles)]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            return dict(skipped=f"the trace run ended with {run.returncode}", tail=run.stderr[-400:])
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as fh:
                rows += list(csv.DictReader(fh))
        out, want = {}, kernel_bytes(n, m)
        for r in rows:
            name, key = r.get("Name", ""), None
            if "mdot_f32_kernel" in name:
                key = "mdot_f32_kernel"
            elif "iter_maxpy_uhead_kernel" in name:
                key = "iter_maxpy_uhead_kernel_f32" if "float" in name else "iter_maxpy_uhead_kernel_f64"
            elif "mdot_kernel" in name:
                key = "mdot_kernel"
            if key is None:
                continue
            calls, total = int(r["Calls"]), float(r["TotalDurationNs"])
            e = out.setdefault(key, dict(calls=0, total_ns=0.0))
            e["calls"] += calls
            e["total_ns"] += total
        for key, e in out.items():
            e["mean_us"] = round(e["total_ns"] / e["calls"] / 1e3, 2)
            e["own_bytes_at_mean_j"] = int(want[key])
            e["tb_per_s"] = round(want[key] / (e["total_ns"] / e["calls"]) / 1e3, 3)
            e["total_ns"] = int(e["total_ns"])
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--converge-grid", type=int, default=512)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.grid, a.cycles)
    lines = []
    c, rhs, n, m = context(a.grid)
    times = {k: [] for k in CONFIGS}
    forms, bases = {}, {}
    for k, kw in CONFIGS.items():   # warm-up, and what each configuration resolves to
        cycles_solve(c, rhs, 1, **kw)
        forms[k], bases[k] = c.iteration_form()[0], c.basis_info()
    for _ in range(a.rounds):
        for k, kw in CONFIGS.items():
            times[k].append(cycles_solve(c, rhs, a.cycles, **kw))
    model = byte_model(c, n, m)
    c.close()
    st = {k: stat(v) for k, v in times.items()}
    s, au = st["single"], st["auto"]
    line = dict(mode="basis_us_per_iteration", grid=a.grid, rows=n, m=m, restart=RESTART, cycles=a.cycles, rounds=a.rounds,
                iteration_form=forms, basis={k: dict(precision=v[0], basis_bytes=v[1]) for k, v in bases.items()},
                us_per_iteration=st, raw={k: [round(x, 3) for x in v] for k, v in times.items()}, byte_model=model,
                measured_change_single_vs_auto=round(s["median"] / au["median"] - 1.0, 4),
                measured_change_single_vs_form5=round(s["median"] / st["form5"]["median"] - 1.0, 4),
                bar_single_median_plus_spread_below_auto_median=bool(s["median"] + (s["max"] - s["min"]) < au["median"]))
    print(json.dumps(line), flush=True)
    lines.append(line)
    if not a.no_trace:
        line = dict(mode="basis_kernel_trace", grid=a.grid, cycles=a.cycles, kernels=trace(a.grid, a.cycles, n, m))
        print(json.dumps(line), flush=True)
        lines.append(line)
    c, rhs, n, m = context(a.converge_grid)
    conv = {}
    for k, kw in CONFIGS.items():
        c.fgmres(rhs, rtol=1e-8, **kw)
        x, info = c.fgmres(rhs, rtol=1e-8, **kw)
        true = float(np.linalg.norm(rhs - c.mult(x)) / np.linalg.norm(rhs))
        conv[k] = dict(its=info["its"], cycles=info["cycles"], reason=info["reason"], solve_ms=round(info["solve_seconds"] * 1e3, 3),
                       true_residual_over_b=float(f"{true:.3e}"))
    c.close()
    line = dict(mode="basis_to_rtol_1e-8", grid=a.converge_grid, rows=n, m=m, solves=conv)
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
