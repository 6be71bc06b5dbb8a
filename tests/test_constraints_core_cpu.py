"""The constraint block's closed forms (csrc/spk_constraints_core.hpp), which the kernels of spk_k_constraints.hip
execute, without a GPU and without ROCm: tests/host/constraints_core_check.cpp runs the kernels' bodies on the CPU for
every grid with sides 3..10 (2-D) and 3..6 (3-D) and every slab of whole node lines or planes -- slabs of boundary
lines only and empty ones included -- and compares B by rows, B^T by rows and the window pointers byte for byte with
what the host chain produces (the generator of spk_assembly.cpp, then localise_and_sort, wide_rows, window_pointers and
transpose_rows of spk_host.cpp).  Compiled with g++ beside those two sources and run as a plain process, once as it is
and once with the address and undefined-behaviour sanitizers.

Then what the new entry points refuse before they need a GPU: the facade's and the runner's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd.solver import constraints_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")
RUNNER = os.path.join(ROOT, "saddle_point_petsc_amd", "saddle_point_run")
SPK_ERR_ARG = -1
# 2-D: sum over my = 3..10 of the slabs [u0, u1), u0 <= u1 <= my, for 8 values of mx; 3-D: the same over mz = 3..6, 16 (mx, my)
CASES = 8 * sum((u + 1) * (u + 2) // 2 for u in range(3, 11)) + 16 * sum((u + 1) * (u + 2) // 2 for u in range(3, 7))


@pytest.mark.parametrize("sanitize", [False, True])
def test_core_reproduces_the_host_chain(tmp_path, sanitize):
    exe = tmp_path / "constraints_core_check"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, "spk_assembly.cpp"),
                           os.path.join(CSRC, "spk_host.cpp"), os.path.join(ROOT, "tests", "host", "constraints_core_check.cpp"),
                           "-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert f"{CASES} cases, 0 failed" in out.stdout
    assert "all constraints core checks passed" in out.stdout


def test_core_header_includes_nothing_from_rocm():
    """spk_constraints_core.hpp: the assembly core and, through it, the standard library only"""
    src = open(os.path.join(CSRC, "spk_constraints_core.hpp")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs == ['"spk_assembly_core.hpp"'], incs


@pytest.mark.parametrize("grid", [(5, 4, 0), (4, 3, 5)])
def test_host_reference_is_the_generators_block(grid):
    """spk_host_constraints_csr (the reference of the GPU tests) against the generator's block through numpy: the
    localised columns, the stable transpose, the window pointers as searchsorted"""
    mx, my, mz = grid
    B, _ = S.AssembleOperator_Constraints3D(mx, my, mz) if mz else S.AssembleOperator_Constraints(mx, my)
    dof, m = (3, 6) if mz else (2, 4)
    unit = dof * mx * (my if mz else 1)
    for rb, re in [(0, B.ncols), (unit, 3 * unit), (0, unit)]:
        Bs, _ = (S.AssembleOperator_Constraints3D(mx, my, mz, rb, re) if mz else S.AssembleOperator_Constraints(mx, my, rb, re))
        got = constraints_csr(mx, my, mz, rb, re)
        col = Bs.colidx - rb
        assert np.array_equal(got["b_colidx"], col) and got["b_val"].tobytes() == Bs.val.tobytes()
        rows = np.repeat(np.arange(m), np.diff(Bs.rowptr))
        order = np.argsort(col, kind="stable")
        assert np.array_equal(got["bt_colidx"], rows[order]) and got["bt_val"].tobytes() == Bs.val[order].tobytes()
        assert np.array_equal(got["bt_rowptr"], np.concatenate([[0], np.cumsum(np.bincount(col, minlength=re - rb))]))
        assert got["win"] == 1024 and got["nwin"] == 1 and got["winptr"].shape == (2, m)
        assert np.array_equal(got["winptr"][0], Bs.rowptr[:-1]) and np.array_equal(got["winptr"][1], Bs.rowptr[1:])


def test_facade_refusals_that_need_no_gpu():
    with S.KSP(0) as ksp:
        with pytest.raises(ValueError, match="device"):
            ksp.setOperatorsLaplace(9, 9, B="host")
        with pytest.raises(ValueError, match="device"):
            ksp.setOperatorsLaplace3D(5, 5, 5, B="gpu")
        with pytest.raises(S.SpkError) as e:        # mz = 0 is the 2-D entry point's
            ksp.setOperatorsLaplace3D(5, 5, 0, B="device")
        assert e.value.code == SPK_ERR_ARG and "mz = 0" in str(e.value)
    assert S._lib.lib.SpkKSPSetOperatorsLaplaceConstrained(None, 9, 9, None, None) == SPK_ERR_ARG
    assert S._lib.lib.spk_set_block_constraints(None, 9, 9, 0, None) == SPK_ERR_ARG
    assert S._lib.lib.spk_get_constraints_seconds(None, C.byref(C.c_double())) == SPK_ERR_ARG
    with pytest.raises(S.SpkError):
        constraints_csr(9, 9, 0, 3, 18)             # not whole node lines
    with pytest.raises(S.SpkError):
        constraints_csr(2, 9)                       # a side of 2


@pytest.mark.parametrize("args,words", [
    (["-spk_constraints", "device"], ["-spk_constraints device", "-spk_assembly device"]),
    (["-spk_constraints", "device", "-spk_assembly", "host"], ["-spk_assembly device"]),
    (["-spk_constraints", "gpu", "-spk_assembly", "device"], ["-spk_constraints gpu", "host | device"]),
    (["-spk_constraints", "device", "-spk_assembly", "device", "-saddle", "0"], ["-saddle"]),
])
def test_runner_refusals_that_need_no_gpu(tmp_path, args, words):
    out = subprocess.run([RUNNER, "-da_grid_x", "9", "-da_grid_y", "9", "-no_vtk"] + args, capture_output=True, text=True,
                         cwd=tmp_path, timeout=60)
    assert out.returncode == 1 and out.stdout == "", out.stdout + out.stderr
    for w in words:
        assert w in out.stderr, out.stderr
