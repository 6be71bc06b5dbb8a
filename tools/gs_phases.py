#!/usr/bin/env python3
"""Phase table of form 7's fused Gram-Schmidt launch (gs_fused_kernel) from a library built with `make GS_STAMPS=1`
(csrc/spk_gs_stamps.hpp):
    python tools/gs_phases.py [--grid 1024] [--grid-y 0] [--pc schur-full|jacobi] [--cycles 3] [--label TEXT] [--straggler]
Runs whole restart cycles of FGMRES(30) (rtol 0), reads the time stamps every workgroup's thread 0 took in the LAST cycle
and prints, per position loc in the cycle, the median and the longest duration of each phase over the launch's workgroups
(us), the skew between the first and the last workgroup at "MDot tiles done", and the launch from its first entry to its
last workgroup's end of kernel B's tiles.  A phase runs from the stamp before it:
    dispatch   first workgroup's kernel entry -> this workgroup's entry
    loads1     entry -> the first tile's first group of loads returned (and summed)
    tiles      -> VecMDot's tiles done
    wsum+pub   -> wave sums, cross-wave sums, partials published
    totals     -> the totals this workgroup needs seen (the reducer's chain and every slower workgroup are in here)
    prologue   -> kernel B's scalar prologue done
    B tiles    -> kernel B's tiles done"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import saddle_point_petsc_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=1024)
ap.add_argument("--grid-y", type=int, default=0)
ap.add_argument("--pc", default="schur-full", choices=["schur-full", "jacobi"])
ap.add_argument("--restart", type=int, default=30)
ap.add_argument("--cycles", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--straggler", action="store_true",
                help="per loc also: the workgroup that is last at 'MDot tiles done', its gap to the second-last and to the median")
a = ap.parse_args()

mx, my = a.grid, a.grid_y or a.grid
A, f = S.AssembleOperator_Laplace(mx, my)
with S.Context(0) as c:
    c.set_block(S.BLOCK_A00, A)
    if a.pc == "schur-full":
        B, g = S.AssembleOperator_Constraints(mx, my)
        c.set_block(S.BLOCK_A10, B)
        c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL)
        rhs = np.concatenate([f, g])
        m = B.nrows
    else:
        c.pc_setup(S.PC_JACOBI)
        rhs, m = f, 0
    c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=a.cycles * a.restart, restart=a.restart)
    form = c.iteration_form()[0]
    st = c.debug_gs_stamps()
if form != 7:
    sys.exit(f"gs_phases: this solve ran iteration form {form}, not the fused launch (form 7)")

names = ["dispatch", "loads1", "tiles", "wsum+pub", "totals", "prologue", "B tiles"]
print(f"# {mx} x {my} {a.pc}, FGMRES({a.restart}), last of {a.cycles} whole cycles; gs_fused_kernel per position loc; us, 100 MHz stamps of"
      f" thread 0 of each of the launch's workgroups{'; ' + a.label if a.label else ''}")
print("# median / max over workgroups of each phase; skew = last - first workgroup at 'MDot tiles done'; launch = first entry -> last 'B tiles' stamp")
print("loc  nv NG | " + " | ".join(f"{n:>13s}" for n in names) + " |  skew | launch")
tot = np.zeros(len(names))
rows = 0
last = []   # --straggler: (loc, workgroup, XCD = workgroup % 8, gap to the second-last, gap to the median), us
for loc in range(64):
    t = st[loc].astype(np.int64)
    live = t[:, 6] > 0
    if not live.any():
        continue
    if (t[live, 1] < t[live, 0]).any():
        # a launch enqueued behind the solve's end and gated off by the device stamped its entry over this row
        print(f"{loc:3d}  (entry stamps overwritten by a gated launch behind the end of the solve)")
        continue
    wgs = np.flatnonzero(live)
    t = t[live] / 100.0
    if t.shape[0] > 1:
        order = np.argsort(t[:, 2], kind="stable")
        last.append((loc, int(wgs[order[-1]]), t[order[-1], 2] - t[order[-2], 2], t[order[-1], 2] - np.median(t[:, 2])))
    ph = np.empty((t.shape[0], 7))
    ph[:, 0] = t[:, 0] - t[:, 0].min()
    ph[:, 1:] = np.diff(t[:, :7], axis=1)
    med, mx_ = np.median(ph, axis=0), ph.max(axis=0)
    nv = loc + 1
    ng = max(1, (nv + m + 7) // 8)
    print(f"{loc:3d} {nv:3d} {ng:2d} | " + " | ".join(f"{md:6.2f} {xx:6.2f}" for md, xx in zip(med, mx_)) +
          f" | {t[:, 2].max() - t[:, 2].min():5.2f} | {t[:, 6].max() - t[:, 0].min():6.2f}")
    tot += med
    rows += 1
if rows:
    print(f"sum of medians over {rows} launches: " + ", ".join(f"{n} {v:.1f}" for n, v in zip(names, tot)) + " us")
if a.straggler and last:
    print("# the workgroup that is last at 'MDot tiles done' (XCD = workgroup mod 8), its gap to the second-last one and to the median workgroup, us")
    print("loc | last wg xcd | to 2nd-last | to median")
    for loc, wg, g2, gm in last:
        print(f"{loc:3d} | {wg:7d} {wg % 8:3d} | {g2:11.2f} | {gm:9.2f}")
    who = np.bincount([wg for _, wg, _, _ in last], minlength=1)
    top = np.argsort(-who, kind="stable")[:5]
    print("most often last: " + ", ".join(f"workgroup {w} ({who[w]} of {len(last)})" for w in top if who[w]))
