"""The bytes of one application of the multigrid cycle on every route of the host walk (csrc/spk_amg_cycle.cpp) against
tests/golden/mg_cycle_parent.npz, recorded on an MI355X by tools/record_mg_cycle_golden.py on the commit before the FP64 and
the FP32 route came to share one typed walk.  The other FP32 cycle tests hold the device to numpy within a tolerance, under
which a wrong coefficient index or a swapped buffer could stay; here every byte counts.

Shapes (tests/test_gpu_mg_operator.py's SHAPES, coarse_eq_limit 10, device set-up; the smallest with a level strictly between
level 0 and the coarsest in each node size) and cases: the recorder's, see its docstring -- FP32 levels under V and W, as
launches and, from 50 rows on, inside the fused tail (on 33x9 and 12x10any FP32 levels then run on both sides of the tail's
first level); the FP64 stencil route under W; the FP64 CSR route with matrix-free transfers under V, and on the sparse
products with stored transfers under W with the fused tail; on the two Laplace operators of bs 2 the aggregation hierarchy
under V and W (stored CSR levels throughout)."""
import importlib.util
import os

import numpy as np
import pytest

import saddle_point_petsc_amd as S
from test_gpu_mg_operator import SHAPES, _problem, _vec

# the recorder states the shapes and the cases once, for itself and for this test
_spec = importlib.util.spec_from_file_location(
    "record_mg_cycle_golden", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_mg_cycle_golden.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mg_cycle_parent.npz")
ROWS = {"33x9": [594, 170, 54, 30, 18], "12x10any": [240, 84, 32, 18], "6x4x3any": [216, 108, 81], "five17x9": [153, 45, 15, 9]}
TAIL_FIRST_50 = {"33x9": 3, "12x10any": 2, "6x4x3any": -1, "five17x9": 1}   # the first level of at most 50 rows below level 0


def test_the_cases_are_the_shapes_of_the_operator_tests():
    assert os.path.getsize(GOLDEN) < 100 * 1024
    gold = np.load(GOLDEN)
    keys = {f"x__{name}" for name in R.SHAPES}
    for name, (grid, bs, sides) in R.SHAPES.items():
        assert SHAPES[name][:3] == (grid, bs, sides)
        keys |= {f"{name}__{R.options(name, case)[1]}" for case in R.cases(name)}
        for case in ("aggregation_v", "aggregation_w"):
            assert (case in R.cases(name)) == (name in ("33x9", "12x10any"))
    assert set(gold.files) == keys
    assert len(R.CASES) == 5 and list(R.SAME_AS) == ["single_w_fused50"] and R.SAME_AS["single_w_fused50"][0] == "single_w"


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_one_application_gives_the_recorded_bytes(name):
    A, _ = _problem(name)
    x = _vec(A.nrows, R.SEED)
    gold = np.load(GOLDEN)
    assert gold[f"x__{name}"].tobytes() == x.tobytes()
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        for case in R.cases(name):
            amg, key = R.options(name, case)
            c.pc_setup(S.PC_JACOBI, amg=amg)
            info = c.amg_info()
            y, y2 = c.pc_apply(x), c.pc_apply(x)
            if case not in R.AGGREGATION:
                assert info["rows"] == ROWS[name]
                assert info["precision"] == (S.AMG_PRECISION_SINGLE if case.startswith("single") else S.AMG_PRECISION_DOUBLE)
                assert info["tail_first"] == (TAIL_FIRST_50[name] if "fused" in case else -1), (name, case)
            ref = gold[f"{name}__{key}"]
            print(f"{name} {case}: rows {info['rows']} tail_first {info['tail_first']}, {np.abs(y - ref).max():.3e} off the recorded bytes")
            assert y.tobytes() == ref.tobytes(), f"{name} {case}: {np.abs(y - ref).max():.3e} off the recorded bytes"
            assert y2.tobytes() == y.tobytes(), f"{name} {case}: a second application gave other bytes"
