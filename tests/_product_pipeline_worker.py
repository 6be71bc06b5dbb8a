"""What tests/test_gpu_product_pipeline.py computes on one dof-2 grid, and the child process that computes it under a
developer knob that is read once per process (SPK_DICT2_WGS, the workgroup count of the pipelined row-type product):

    python _product_pipeline_worker.py MX MY OUT.npz

Per layout (the default row types + codes, and SPK_SPMV_FORMAT=csr):
  y_plain              y = A x through mult on a context that holds A alone         (ACC = 0, BT = 0)
  jac_x, jac_hist      FGMRES(5) form 5, Jacobi, 12 iterations on A                 (ACC = 0 with the rider)
  y_bt                 K [x; lambda] through mult on the saddle system              (BT = 1)
  full_x, full_hist    FGMRES(5) form 5, Schur FULL, 12 iterations on the saddle system (y += A x with the rider)
"""
import os
import sys

import numpy as np

LAYOUTS = {"dict": None, "csr": "csr"}
SOLVE = dict(rtol=1e-30, max_it=12, restart=5, iteration_form=5)


def inputs(spk, mx, my):
    A, f = spk.AssembleOperator_Laplace(mx, my)
    B, g = spk.AssembleOperator_Constraints(mx, my)
    rng = np.random.default_rng(1000 * mx + my)
    return A, f, B, g, rng.uniform(-1.0, 1.0, A.nrows), rng.uniform(-1.0, 1.0, A.nrows + B.nrows)


def run_grid(spk, mx, my):
    """{layout_key: array}: see the module docstring; 'dict_format' / 'csr_format' hold spmv_info()['format']"""
    A, f, B, g, x, xs = inputs(spk, mx, my)
    saved = os.environ.pop("SPK_SPMV_FORMAT", None)
    out = {}
    try:
        for name, fmt in LAYOUTS.items():
            if fmt is None:
                os.environ.pop("SPK_SPMV_FORMAT", None)
            else:
                os.environ["SPK_SPMV_FORMAT"] = fmt
            with spk.Context(0) as c:
                c.set_block(spk.BLOCK_A00, A)
                out[name + "_format"] = np.array(c.spmv_info()["format"])
                out[name + "_y_plain"] = c.mult(x)
                c.pc_setup(spk.PC_JACOBI)
                sol, info = c.fgmres(f, **SOLVE)
                out[name + "_jac_x"], out[name + "_jac_hist"] = sol, np.asarray(info["history"])
            with spk.Context(0) as c:
                c.set_block(spk.BLOCK_A00, A)
                c.set_block(spk.BLOCK_A10, B)
                out[name + "_y_bt"] = c.mult(xs)
                c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
                sol, info = c.fgmres(np.concatenate([f, g]), **SOLVE)
                out[name + "_full_x"], out[name + "_full_hist"] = sol, np.asarray(info["history"])
    finally:
        os.environ.pop("SPK_SPMV_FORMAT", None)
        if saved is not None:
            os.environ["SPK_SPMV_FORMAT"] = saved
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import saddle_point_petsc_amd as S
    np.savez(sys.argv[3], **run_grid(S, int(sys.argv[1]), int(sys.argv[2])))
