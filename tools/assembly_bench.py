#!/usr/bin/env python3
"""KSPSetOperators for A00, two routes in one process: (a) the host assembler (16 threads) followed by set_block of
its arrays, (b) set_block_laplace, which assembles the slab on the device.  One warm-up of each route per grid, then
`--reps` alternating repetitions; every time is a host clock around work that ends in a device synchronise (both calls
are synchronous at return).  Prints one JSON line per grid and a table.

  python tools/assembly_bench.py [--grids 256 512 1024] [--reps 5] [--out profiles/assembly_256_512_1024.jsonl]
  python tools/assembly_bench.py --3d [--grids3d 64x64x64 128x128x32 256x256x32] [--reps 5]

--3d: the 3-D generator (AssembleOperator_Laplace3D against set_block_laplace3d); 256 x 256 x 32 is one rank's share of
256^3 in eight z-slabs; the host assembler takes 1.3 s there, so every size gets the same --reps.  Before a size is timed, the two warmed-up contexts must agree byte for byte in spmv_info() and in
y = A x; the tool stops otherwise.  Each 3-D line says whether the device route's median plus its spread lies below the
median of the host route's set_block alone.

--constraints: the saddle block instead of A00 -- (a) the host generator (AssembleOperator_Constraints[3D], serial)
followed by set_block(A10) of its arrays, (b) set_block_constraints, which writes B, B^T and the window pointers on the
device.  Both contexts hold the device-assembled A00 of the grid; after the warm-up their products of a saddle vector
must agree byte for byte.  With --3d the 3-D block over --grids3d.  The bar: the device route's median plus its min-to-max
spread at or below the median of the host route's set_block(A10) alone.  The bytes written -- 12 B per entry of B and of
B^T, B^T's row pointers, the window pointers -- are a byte-model figure, not a bandwidth claim.

  python tools/assembly_bench.py --constraints [--grids 256 512 1024] [--out profiles/constraints_256_512_1024.jsonl]
  python tools/assembly_bench.py --constraints --3d --grids3d 64x64x64 256x256x32 [--out profiles/constraints3d_64_256x256x32.jsonl]

The kernel's share of 8 TB/s is a byte-model figure -- 12 B per stored non-zero plus row pointers and f written, kappa
read -- of a kernel that is compute-heavy (an 8 x 8 element matrix per element and workgroup): it says how far the
assembly is from the cost of merely writing its output, not how well it uses the memory system."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import saddle_point_petsc_amd as S  # noqa: E402

HBM_BYTES_PER_SECOND = 8e12


def stat(v):
    return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6))


def host_route(c, m, threads):
    """m: the side of a square 2-D grid, or (mx, my, mz)"""
    t0 = time.perf_counter()
    A, f = S.AssembleOperator_Laplace3D(*m, nthreads=threads) if isinstance(m, tuple) else S.AssembleOperator_Laplace(m, nthreads=threads)
    t1 = time.perf_counter()
    c.set_block(S.BLOCK_A00, A)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, t2 - t0


def device_route(c, m, kappa, fdev):
    t0 = time.perf_counter()
    if isinstance(m, tuple):
        c.set_block_laplace3d(*m, kappa=kappa, rhs=fdev)
    else:
        c.set_block_laplace(m, kappa=kappa, rhs=fdev)
    t1 = time.perf_counter()
    return t1 - t0, c.assembly_seconds()


def bench3d(a):
    lines = []
    for name in a.grids3d:
        g = tuple(int(v) for v in name.split("x"))
        n = 3 * g[0] * g[1] * g[2]
        nnz = 9 * (3 * g[0] - 2) * (3 * g[1] - 2) * (3 * g[2] - 2)
        ne = (g[0] - 1) * (g[1] - 1) * (g[2] - 1)
        reps = a.reps
        with S.Context(0) as ch, S.Context(0) as cd:
            fdev = cd.vec_create(n=n)
            kappa = cd.vec_create(np.full(ne, 1.5)) if a.kappa else None
            host_route(ch, g, a.threads)
            device_route(cd, g, None, fdev)
            # the two routes leave the same operator: layout and product, byte for byte (at real size this is where the
            # kernel's 64-bit offsets are exercised)
            x = np.sin(0.37 * np.arange(n))
            same = cd.spmv_info() == ch.spmv_info() and cd.sizes() == ch.sizes() and cd.mult(x).tobytes() == ch.mult(x).tobytes()
            if not same:
                raise SystemExit(f"{name}: the device-assembled operator differs from the host-assembled one")
            if kappa is not None:
                device_route(cd, g, kappa, fdev)
            asm, setb, both, dev, kern = [], [], [], [], []
            for _ in range(reps):
                t = host_route(ch, g, a.threads)
                asm.append(t[0]), setb.append(t[1]), both.append(t[2])
                t = device_route(cd, g, kappa, fdev)
                dev.append(t[0]), kern.append(t[1])
            cd.vec_destroy(fdev)
            if kappa is not None:
                cd.vec_destroy(kappa)
        model = 12 * nnz + 4 * (n + 1) + 8 * n + (8 * ne if a.kappa else 0)
        d, sb = stat(dev), stat(setb)
        line = dict(mode="assembly3d", grid=name, rows=n, nnz=nnz, reps=reps, threads=a.threads, kappa=bool(a.kappa),
                    host_assemble_seconds=stat(asm), host_set_block_seconds=sb, host_total_seconds=stat(both),
                    device_set_block_laplace3d_seconds=d, device_kernel_seconds=stat(kern), model_bytes=model,
                    kernel_byte_model_share_of_8TBs=round(model / statistics.median(kern) / HBM_BYTES_PER_SECOND, 4),
                    device_median_plus_spread_below_host_set_block_median=bool(d["median"] + (d["max"] - d["min"]) < sb["median"]),
                    same_layout_and_product=bool(same),
                    raw=dict(host_set_block=[round(v, 6) for v in setb], device=[round(v, 6) for v in dev], kernel=[round(v, 6) for v in kern]))
        print(json.dumps(line), flush=True)
        lines.append(line)
    print("\n| grid | reps | host assembly (s) | host set_block (s) | host both (s) | device set_block_laplace3d (s) | kernel (ms) | byte model / 8 TB/s | bar met |")
    print("|---|---|---|---|---|---|---|---|---|")
    fmt = lambda s: f"{s['median']:.4f} ({s['min']:.4f}..{s['max']:.4f})"  # noqa: E731
    for ln in lines:
        k = ln["device_kernel_seconds"]
        print(f"| {ln['grid']} | {ln['reps']} | {fmt(ln['host_assemble_seconds'])} | {fmt(ln['host_set_block_seconds'])} | {fmt(ln['host_total_seconds'])} | "
              f"{fmt(ln['device_set_block_laplace3d_seconds'])} | {k['median'] * 1e3:.3f} ({k['min'] * 1e3:.3f}..{k['max'] * 1e3:.3f}) | "
              f"{ln['kernel_byte_model_share_of_8TBs']:.3f} | {'yes' if ln['device_median_plus_spread_below_host_set_block_median'] else 'no'} |")
    return lines


def bench_constraints(a):
    lines = []
    grids = [tuple(int(v) for v in name.split("x")) for name in a.grids3d] if a.three_d else [(m, m, 0) for m in a.grids]
    for g in grids:
        mx, my, mz = g
        three = mz != 0
        name = "x".join(str(v) for v in g) if three else f"{mx}x{my}"
        dof, m = (3, 6) if three else (2, 4)
        n = dof * mx * my * (mz if three else 1)

        def host_b(c):
            t0 = time.perf_counter()
            B, _ = S.AssembleOperator_Constraints3D(mx, my, mz) if three else S.AssembleOperator_Constraints(mx, my)
            t1 = time.perf_counter()
            c.set_block(S.BLOCK_A10, B)
            t2 = time.perf_counter()
            return t1 - t0, t2 - t1, t2 - t0, int(B.rowptr[-1])

        def device_b(c, gdev):
            t0 = time.perf_counter()
            c.set_block_constraints(mx, my, mz, rhs=gdev)
            t1 = time.perf_counter()
            return t1 - t0, c.constraints_seconds()

        with S.Context(0) as ch, S.Context(0) as cd:
            for c in (ch, cd):
                c.set_block_laplace3d(mx, my, mz) if three else c.set_block_laplace(mx, my)
            gdev = cd.vec_create(n=8)
            nnz = host_b(ch)[3]
            device_b(cd, gdev)
            x = np.sin(0.37 * np.arange(n + m))
            same = cd.sizes() == ch.sizes() and cd.mult(x).tobytes() == ch.mult(x).tobytes()
            if not same:
                raise SystemExit(f"{name}: the device-written constraint block differs from the host-fed one")
            gen, setb, both, dev, kern = [], [], [], [], []
            for _ in range(a.reps):
                t = host_b(ch)
                gen.append(t[0]), setb.append(t[1]), both.append(t[2])
                t = device_b(cd, gdev)
                dev.append(t[0]), kern.append(t[1])
            cd.vec_destroy(gdev)
        win = 8192
        while (n + win - 1) // win > 2048:
            win *= 2
        while win > 1024 and (n + win - 1) // win < 128:
            win //= 2
        model = 24 * nnz + 4 * (n + 1) + 4 * ((n + win - 1) // win + 1) * m
        d, sb = stat(dev), stat(setb)
        line = dict(mode="constraints3d" if three else "constraints", grid=name, cols=n, rows=m, nnz=nnz, reps=a.reps,
                    host_generator_seconds=stat(gen), host_set_block_a10_seconds=sb, host_total_seconds=stat(both),
                    device_set_block_constraints_seconds=d, device_kernel_seconds=stat(kern), model_bytes_written=model,
                    device_median_plus_spread_at_or_below_host_set_block_median=bool(d["median"] + (d["max"] - d["min"]) <= sb["median"]),
                    same_sizes_and_product=bool(same),
                    raw=dict(host_generator=[round(v, 6) for v in gen], host_set_block=[round(v, 6) for v in setb],
                             device=[round(v, 6) for v in dev], kernel=[round(v, 6) for v in kern]))
        print(json.dumps(line), flush=True)
        lines.append(line)
    print("\n| grid | entries | host generator (s) | host set_block(A10) (s) | host both (s) | device set_block_constraints (s) | kernels (ms) | bytes written (MB) | bar met |")
    print("|---|---|---|---|---|---|---|---|---|")
    fmt = lambda s: f"{s['median']:.4f} ({s['min']:.4f}..{s['max']:.4f})"  # noqa: E731
    for ln in lines:
        k = ln["device_kernel_seconds"]
        print(f"| {ln['grid']} | {ln['nnz']} | {fmt(ln['host_generator_seconds'])} | {fmt(ln['host_set_block_a10_seconds'])} | {fmt(ln['host_total_seconds'])} | "
              f"{fmt(ln['device_set_block_constraints_seconds'])} | {k['median'] * 1e3:.3f} ({k['min'] * 1e3:.3f}..{k['max'] * 1e3:.3f}) | "
              f"{ln['model_bytes_written'] / 1e6:.1f} | {'yes' if ln['device_median_plus_spread_at_or_below_host_set_block_median'] else 'no'} |")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--kappa", action="store_true", help="the device route with a coefficient array resident on the device")
    ap.add_argument("--out", default=None)
    ap.add_argument("--3d", dest="three_d", action="store_true", help="the 3-D generator (see above)")
    ap.add_argument("--grids3d", nargs="+", default=["64x64x64", "128x128x32", "256x256x32"])
    ap.add_argument("--constraints", action="store_true", help="the saddle block B instead of A00 (see above)")
    a = ap.parse_args()
    if a.three_d or a.constraints:
        lines = bench_constraints(a) if a.constraints else bench3d(a)
        if a.out:
            with open(a.out, "w") as fh:
                for ln in lines:
                    fh.write(json.dumps(ln) + "\n")
        return
    lines = []
    for m in a.grids:
        n, nnz = S.grid_sizes(m)
        with S.Context(0) as ch, S.Context(0) as cd:
            fdev = cd.vec_create(n=n)
            kappa = cd.vec_create(np.full((m - 1) * (m - 1), 1.5)) if a.kappa else None
            host_route(ch, m, a.threads)
            device_route(cd, m, kappa, fdev)
            asm, setb, both, dev, kern = [], [], [], [], []
            for _ in range(a.reps):
                t = host_route(ch, m, a.threads)
                asm.append(t[0]), setb.append(t[1]), both.append(t[2])
                t = device_route(cd, m, kappa, fdev)
                dev.append(t[0]), kern.append(t[1])
            same = cd.spmv_info() == ch.spmv_info() and cd.sizes() == ch.sizes()
            cd.vec_destroy(fdev)
            if kappa is not None:
                cd.vec_destroy(kappa)
        model = 12 * nnz + 4 * (n + 1) + 8 * n + (8 * (m - 1) ** 2 if a.kappa else 0)
        d, sb = stat(dev), stat(setb)
        line = dict(mode="assembly", grid=m, rows=n, nnz=nnz, reps=a.reps, threads=a.threads, kappa=bool(a.kappa),
                    host_assemble_seconds=stat(asm), host_set_block_seconds=sb, host_total_seconds=stat(both),
                    device_set_block_laplace_seconds=d, device_kernel_seconds=stat(kern), model_bytes=model,
                    kernel_byte_model_share_of_8TBs=round(model / statistics.median(kern) / HBM_BYTES_PER_SECOND, 4),
                    device_median_plus_spread_below_host_set_block_median=bool(d["median"] + (d["max"] - d["min"]) < sb["median"]),
                    same_layout=bool(same))
        print(json.dumps(line), flush=True)
        lines.append(line)
    print("\n| grid | host assembly (s) | host set_block (s) | host both (s) | device set_block_laplace (s) | kernels (ms) | byte model / 8 TB/s |")
    print("|---|---|---|---|---|---|---|")
    fmt = lambda s: f"{s['median']:.4f} ({s['min']:.4f}..{s['max']:.4f})"  # noqa: E731
    for ln in lines:
        k = ln["device_kernel_seconds"]
        print(f"| {ln['grid']}² | {fmt(ln['host_assemble_seconds'])} | {fmt(ln['host_set_block_seconds'])} | {fmt(ln['host_total_seconds'])} | "
              f"{fmt(ln['device_set_block_laplace_seconds'])} | {k['median'] * 1e3:.3f} ({k['min'] * 1e3:.3f}..{k['max'] * 1e3:.3f}) | "
              f"{ln['kernel_byte_model_share_of_8TBs']:.3f} |")
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
