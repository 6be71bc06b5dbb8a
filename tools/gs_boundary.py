#!/usr/bin/env python3
"""The fused Gram-Schmidt launch (gs_fused_kernel) per position loc in the restart cycle, two builds side by side, from
rocprofv3 CSV output of `bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline` (restart 30, 4 constraint rows):
    tools/gs_boundary.py TRACE_A TRACE_B [PMC_A PMC_B] [--names parent,this]
TRACE_*: directories of `rocprofv3 --kernel-trace --stats --output-format csv` runs; PMC_*: of `rocprofv3 --pmc FETCH_SIZE
--output-format csv` runs of their own (no tracing beside the counters).  The launches are put in dispatch order; a whole
cycle is 29 consecutive launches whose accumulator groups NG (the kernel's first template argument) run 1 .. 5 as loc
0 .. 28 does.  Median over the whole cycles per loc.  Bytes: FETCH_SIZE x 2 (gfx950 counts 64 B per 128-B request of a
16 B/lane read) plus the 48 MiB the launch writes; intercept = time less those bytes at 6.8 TB/s (the slope of the launch
itself within one NG), for the first loc of every NG."""
import collections
import csv
import glob
import os
import re
import statistics
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--names")]
names = ["parent", "this"]
for a in sys.argv[1:]:
    if a.startswith("--names="):
        names = a.split("=", 1)[1].split(",")
if len(args) not in (2, 4):
    sys.exit(__doc__)
M, RESTART = 4, 30
NG_OF = [max(1, (loc + 1 + M + 7) // 8) for loc in range(RESTART - 1)]


def rows(d, pattern):
    f = sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True))
    if not f:
        sys.exit(f"gs_boundary: no {pattern} under {d}")
    return list(csv.DictReader(open(f[0])))


def cycles(seq):
    """seq: [(NG, value)] in dispatch order -> per loc, the values of the whole cycles"""
    per = collections.defaultdict(list)
    i, n = 0, 0
    while i + len(NG_OF) <= len(seq):
        if [s[0] for s in seq[i:i + len(NG_OF)]] == NG_OF:
            for loc in range(len(NG_OF)):
                per[loc].append(seq[i + loc][1])
            i += len(NG_OF)
            n += 1
        else:
            i += 1
    return per, n


def fused(rs, value):
    seq = []
    for r in sorted(rs, key=lambda r: int(r["Dispatch_Id"])):
        m = re.search(r"gs_fused(?:_tail)?_kernel<(\d)", r["Kernel_Name"])
        if m:
            seq.append((int(m.group(1)), value(r)))
    return cycles(seq)


t, nc = [], []
for d in args[:2]:
    per, n = fused(rows(d, "*kernel_trace.csv"), lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    t.append({loc: statistics.median(v) for loc, v in per.items()})
    nc.append(n)
b = None
if len(args) == 4:
    b = []
    for d in args[2:]:
        rs = [r for r in rows(d, "*counter_collection.csv") if r["Counter_Name"] == "FETCH_SIZE"]
        per, _ = fused(rs, lambda r: float(r["Counter_Value"]))
        b.append({loc: 2.0 * statistics.median(v) / 1024.0 for loc, v in per.items()})   # KiB -> MiB, x 2
print(f"# gs_fused_kernel per loc: {names[0]} ({nc[0]} whole cycles) against {names[1]} ({nc[1]}); us, median per loc"
      + ("; MiB read = FETCH_SIZE x 2, median per loc, a run of its own per build" if b else ""))
print(f"loc  nv NG | {names[0]+'_us':>10s} {names[1]+'_us':>9s} {'diff_us':>8s}" + (f" | {names[0]+'_MiB':>10s} {names[1]+'_MiB':>9s}" if b else ""))
sa = sb = 0.0
for loc in range(len(NG_OF)):
    if loc not in t[0] or loc not in t[1]:
        continue
    sa += t[0][loc]
    sb += t[1][loc]
    line = f"{loc:3d} {loc + 1:3d} {NG_OF[loc]:2d} | {t[0][loc]:10.2f} {t[1][loc]:9.2f} {t[1][loc] - t[0][loc]:8.2f}"
    if b:
        line += f" | {b[0].get(loc, float('nan')):10.1f} {b[1].get(loc, float('nan')):9.1f}"
    print(line)
print(f"sum over loc 0..{len(NG_OF) - 1}: {names[0]} {sa:.2f} us, {names[1]} {sb:.2f} us ({(sb - sa) / len(NG_OF):+.2f} us per launch, {100 * (sb - sa) / sa:+.2f} %)")
if b:
    print("# intercept per NG at its first loc: measured us less (MiB read + 48 MiB written) at 6.8 TB/s")
    print("NG loc | " + " | ".join(f"{n+' us':>9s} {'bytes us':>8s} {'left':>6s}" for n in names))
    for ng in range(1, 6):
        loc = NG_OF.index(ng)
        cells = []
        for k in range(2):
            us = t[k].get(loc, float("nan"))
            by = (b[k].get(loc, float("nan")) + 48.0) * 1048576.0 / 6.8e12 * 1e6
            cells.append(f"{us:9.1f} {by:8.1f} {us - by:6.1f}")
        print(f"{ng:2d} {loc:3d} | " + " | ".join(cells))
