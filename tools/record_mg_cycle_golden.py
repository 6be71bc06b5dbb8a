#!/usr/bin/env python3
"""Records tests/golden/mg_cycle_parent.npz: the bytes of one application of the multigrid cycle (pc_apply) per route of the
host walk (csrc/spk_amg_cycle.cpp), for tests/test_gpu_mg_cycle_bytes.py to hold later commits to:
    python tools/record_mg_cycle_golden.py [--out tests/golden/mg_cycle_parent.npz]
Run on an MI355X on a build of the commit whose bytes are the reference.  Only the public Python API is used, so the script
runs unchanged on any commit that has the options it names.

Shapes: the smallest of tests/test_gpu_mg_operator.py's SHAPES with a level strictly between level 0 and the coarsest in
each node size (hierarchies built with coarse_eq_limit 10, on the device):
  33x9      bs 2, level rows 594/170/54/30/18      12x10any  bs 2, 240/84/32/18
  6x4x3any  bs 3, 216/108/81                       five17x9  bs 1, 153/45/15/9
Per shape, from x = standard_normal(n) of seed 11 (CASES): the FP32 levels under V and W as launches; the FP64 stencil route
under W; the FP64 CSR route with matrix-free transfers under V; the FP64 CSR route on the sparse products with stored
transfers under W with the fused tail.  SAME_AS: options that must give the bytes of another case (the FP32 W-cycle with
a fused tail from 50 rows: on 33x9 and 12x10any FP32 levels then run both as launches and inside the tail); nothing is
stored for them.  On the two Laplace operators of bs 2 also the aggregation hierarchy (host set-up) under V and W: the
stored-CSR levels of the FP64 walk.  The file: x__<shape> and <shape>__<case>."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

SEED = 11
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "mg_cycle_parent.npz")
# name -> (grid, bs, sides)
SHAPES = {"33x9": ((33, 9, 1), 2, "odd"), "12x10any": ((12, 10, 1), 2, "any"), "6x4x3any": ((6, 4, 3), 3, "any"),
          "five17x9": ((17, 9, 1), 1, "odd")}
STENCIL = dict(galerkin="stencil", operator="stencil")
CASES = {
    "single_v": dict(STENCIL, precision="single", cycle="v", tail="launches"),
    "single_w": dict(STENCIL, precision="single", cycle="w", tail="launches"),
    "double_stencil_w": dict(STENCIL, precision="double", cycle="w", tail="launches"),
    "double_csr_v": dict(galerkin="stencil", precision="double", operator="csr", transfer="matrixfree", cycle="v"),
    "double_products_stored_w_fused": dict(precision="double", operator="csr", galerkin="products", transfer="stored", cycle="w",
                                           tail="fused", tail_rows=50),
}
SAME_AS = {"single_w_fused50": ("single_w", dict(STENCIL, precision="single", cycle="w", tail="fused", tail_rows=50))}
AGGREGATION = {"aggregation_v": dict(coarsening="aggregation", setup="host", coarse_eq_limit=10, cycle="v"),
               "aggregation_w": dict(coarsening="aggregation", setup="host", coarse_eq_limit=10, cycle="w")}
AGGREGATION_SHAPES = ("33x9", "12x10any")


def operator(S, name):
    """the operators of tests/test_gpu_mg_operator.py's SHAPES"""
    (mx, my, mz), bs, _ = SHAPES[name]
    if bs == 3:
        return S.AssembleOperator_Laplace3D(mx, my, mz)[0]
    if bs == 2:
        return S.AssembleOperator_Laplace(mx, my)[0]
    import scipy.sparse as sp   # bs 1: tests/test_mg_grid_cpu.py's five_point, the 5-point Laplacian plus a shift
    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])  # noqa: E731
    M = (sp.kron(sp.identity(my), T(mx)) + sp.kron(T(my), sp.identity(mx)) + 0.1 * sp.identity(mx * my)).tocsr()
    M.sort_indices()
    return S.CSR(M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.copy(), mx * my)


def options(name, case):
    """the options of one case on one shape, and the key of the case that holds its bytes"""
    grid, bs, sides = SHAPES[name]
    if case in AGGREGATION:
        return AGGREGATION[case], case
    key, kw = SAME_AS[case] if case in SAME_AS else (case, CASES[case])
    return dict(dict(coarsening="grid", grid=grid, sides=sides, block_size=bs, coarse_eq_limit=10, setup="device"), **kw), key


def cases(name):
    return list(CASES) + list(SAME_AS) + (list(AGGREGATION) if name in AGGREGATION_SHAPES else [])


def vector(n):
    return np.random.default_rng(SEED).standard_normal(n)


def apply_twice(S, c, name, case, x):
    """one application under the case's options, checked against a second one; with the hierarchy's description"""
    amg, _ = options(name, case)
    c.pc_setup(S.PC_JACOBI, amg=amg)
    y, y2 = c.pc_apply(x), c.pc_apply(x)
    assert y.tobytes() == y2.tobytes(), f"{name} {case}: a second application gave other bytes"
    return y, c.amg_info()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    import saddle_point_petsc_amd as S

    out = {}
    for name in SHAPES:
        A = operator(S, name)
        x = vector(A.nrows)
        out[f"x__{name}"] = x
        with S.Context(0) as c:
            c.set_block(S.BLOCK_A00, A)
            for case in cases(name):
                y, info = apply_twice(S, c, name, case, x)
                key = options(name, case)[1]
                print(f"{name} {case}: rows {info['rows']} tail_first {info['tail_first']} precision {info['precision']} |y| {np.linalg.norm(y):.17g}",
                      flush=True)
                if key != case:
                    assert y.tobytes() == out[f"{name}__{key}"].tobytes(), f"{name} {case}: not the bytes of {key}"
                else:
                    out[f"{name}__{case}"] = y
    np.savez(a.out, **out)
    print(f"{a.out}: {len(out)} arrays, {os.path.getsize(a.out)} bytes")
