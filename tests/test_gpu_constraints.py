"""The constraint block B and g written on the device (spk_set_block_constraints, spk_k_constraints.hip) against the host
route: the kernels' arrays bit for bit through the test hook, the context they leave against the context the host
arrays leave (products, S^, the B D planes, residual histories, the dense S: same bits, same kernels), g, logical
ranks, the refusals, the KSP facade and the runner.

Grids: 3 x 3 (one interior node), 4 x 3, 3 x 5 and 17 x 9; 33 x 17 (1122 local columns: two column windows of 1024);
3 x 3 x 3, 4 x 3 x 5 and 9 x 9 x 9 (2187 columns: three windows).  Slabs: the whole grid, every third of the lines or
planes, and line / plane 0 alone (a slab of boundary nodes only: every row of B empty)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd.solver import constraints_csr

pytestmark = pytest.mark.gpu
GRIDS = [(3, 3, 0), (4, 3, 0), (3, 5, 0), (17, 9, 0), (33, 17, 0), (3, 3, 3), (4, 3, 5), (9, 9, 9)]
SPK_ERR_ARG, SPK_ERR_STATE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("b_colidx", "b_val", "bt_rowptr", "bt_colidx", "bt_val", "winptr")


def slabs(mx, my, mz):
    """(row_begin, row_end): the whole grid, its thirds, and the first line / plane alone"""
    units, unit_rows = (mz, 3 * mx * my) if mz else (my, 2 * mx)
    cuts = {(0, units), (0, 1)} | {(units * t // 3, units * (t + 1) // 3) for t in range(3)}
    return sorted((a * unit_rows, b * unit_rows) for a, b in cuts)


@functools.lru_cache(maxsize=None)
def host(mx, my, mz, rb, re):
    """the host chain's arrays, computed once per case"""
    return constraints_csr(mx, my, mz, rb, re)


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def same_arrays(got, want):
    assert (got["win"], got["nwin"]) == (want["win"], want["nwin"])
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("mx,my,mz", GRIDS)
def test_kernel_arrays_are_the_host_chains(ctx, mx, my, mz):
    for rb, re in slabs(mx, my, mz):
        want = host(mx, my, mz, rb, re)
        same_arrays(ctx.assemble_constraints_csr(mx, my, mz, rb, re), want)
    first =host(mx, my, mz, *min(slabs(mx, my, mz), key=lambda s: (s[0], s[1])))
    assert first["b_val"].size == 0 and not first["bt_rowptr"].any()        # line / plane 0 alone: nothing but boundary nodes
    if (mx, my, mz) == (33, 17, 0):
        assert host(33, 17, 0, 0, 1122)["nwin"] == 2
    if (mx, my, mz) == (9, 9, 9):
        assert host(9, 9, 9, 0, 2187)["nwin"] == 3


def test_two_launches_give_the_same_bytes(ctx):
    for mx, my, mz in [(33, 17, 0), (9, 9, 9)]:
        a, b = ctx.assemble_constraints_csr(mx, my, mz), ctx.assemble_constraints_csr(mx, my, mz)
        same_arrays(a, b)


def _x(n):
    return np.sin(0.37 * np.arange(n))


def _pair(grid):
    """two contexts with the device-assembled A00 of the grid: B from the host arrays, and B written on the device"""
    three = len(grid) == 3
    B, g = (S.AssembleOperator_Constraints3D if three else S.AssembleOperator_Constraints)(*grid)
    ch, cd = S.Context(0), S.Context(0)
    f = None
    for c in (ch, cd):
        f = (c.set_block_laplace3d if three else c.set_block_laplace)(*grid, rhs=True)
    ch.set_block(S.BLOCK_A10, B)
    mz = grid[2] if three else 0
    gd = cd.set_block_constraints(grid[0], grid[1], mz, rhs=True)
    assert gd.tobytes() == g.tobytes()                                        # g arrives
    assert cd.constraints_seconds() > 0.0 and ch.constraints_seconds() == 0.0
    return ch, cd, np.concatenate([f, g])


@pytest.mark.parametrize("grid", [(33, 17), (9, 5, 7)])
def test_context_equals_the_host_fed_context(grid):
    ch, cd, rhs = _pair(grid)
    try:
        assert cd.sizes() == ch.sizes() and cd.sizes()["m"] == 2 * len(grid)
        n = rhs.size
        assert np.array_equal(cd.mult(_x(n)), ch.mult(_x(n)))
        got = []
        for c in (ch, cd):
            c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL)
            shat, planes = c.schur_diag(), c.bd_planes()
            hist = c.fgmres(rhs, rtol=0.0, max_it=20)[1]["history"]
            c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL, schur_pre="full")
            got.append((shat, planes, hist, c.schur_matrix()))
        (s0, p0, h0, S0), (s1, p1, h1, S1) = got
        assert np.array_equal(s0, s1) and np.all(s0 > 0.0)
        assert p0 == p1
        assert h0.size == 21 and np.array_equal(h0, h1)
        assert np.array_equal(S0, S1) and np.all(np.diag(S0.reshape(2 * len(grid), -1)) > 0.0)
        assert np.array_equal(cd.mult(_x(n)), ch.mult(_x(n)))
    finally:
        ch.close()
        cd.close()


def _group(P, mx, my, device):
    grp = S.LocalGroup(P)
    out, errs = [None] * P, []
    n = 2 * mx * my

    def work(r):
        try:
            b, e = S.partition_slab(mx, my, r, P)
            with S.Context(0) as c:
                c.comm_init_local(grp, r)
                f = c.set_block_laplace(mx, my, rhs=True)
                if device:
                    g = c.set_block_constraints(mx, my, 0, rhs=True)
                else:
                    Bs, g = S.AssembleOperator_Constraints(mx, my, b, e)
                    c.set_block(S.BLOCK_A10, Bs)
                c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL)
                y = c.mult(np.concatenate([_x(n)[b:e], _x(4)]))
                hist = c.fgmres(np.concatenate([f, g]), rtol=0.0, max_it=20)[1]["history"]
                out[r] = (b, e, y, hist)
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            raise

    th = [threading.Thread(target=work, args=(r,)) for r in range(P)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    alive = [t.is_alive() for t in th]
    grp.close()
    assert not errs and not any(alive), (errs, alive)
    return out


@pytest.mark.parametrize("P", [2, 3])
def test_logical_ranks_match_the_host_fed_group(P):
    mx, my = 33, 17
    dev, hst = _group(P, mx, my, True), _group(P, mx, my, False)
    for (b, e, y, h), (b0, e0, y0, h0) in zip(dev, hst):
        assert (b, e) == (b0, e0)
        assert np.array_equal(y, y0)
        assert h.size == 21 and np.array_equal(h, h0)


def test_refusals_leave_the_previous_block():
    mx, my = 33, 17
    with S.Context(0) as c:
        with pytest.raises(S.SpkError) as e:                                  # before A00
            c.set_block_constraints(mx, my)
        assert e.value.code == SPK_ERR_STATE
        f = c.set_block_laplace(mx, my, rhs=True)
        g = c.set_block_constraints(mx, my, rhs=True)
        rhs = np.concatenate([f, g])
        c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL)
        y0 = c.mult(_x(rhs.size))
        h0 = c.fgmres(rhs, rtol=1e-10)[1]
        assert h0["reason"] > 0
        for bad in [(33, 16, 0),       # a grid that is not A00's
                    (11, 17, 3),       # the 3-D block over the 2-D operator
                    (2, 17, 0),        # a side of 2
                    (33, 17, 2)]:      # a side of 2: mz
            with pytest.raises(S.SpkError) as e:
                c.set_block_constraints(*bad)
            assert e.value.code == SPK_ERR_ARG, bad
            assert c.sizes()["m"] == 4
            assert np.array_equal(c.mult(_x(rhs.size)), y0)
            h = c.fgmres(rhs, rtol=1e-10)[1]                                  # the previous B still solves
            assert h["reason"] == h0["reason"] and np.array_equal(h["history"], h0["history"])
        # the library's own refusal of rows that are not whole node lines, through the hook (the wrapper refuses them first)
        i, d, w = np.zeros(4096, np.int32), np.zeros(4096), C.c_int32()
        rc = S._lib.lib.spk_assemble_constraints_csr(c.h, mx, my, 0, 3, 2 * mx, i, d, i.copy(), i.copy(), d.copy(), C.byref(w), C.byref(w),
                                                     i.copy(), 4096)
        assert rc == SPK_ERR_ARG and "whole node lines" in c.last_error()
        assert c.sizes()["m"] == 4 and np.array_equal(c.mult(_x(rhs.size)), y0)
    with S.Context(0) as c:                                                   # a side of 2 on A00's own grid
        c.set_block_laplace(2, 9)
        y0 = c.mult(_x(36))
        with pytest.raises(S.SpkError) as e:
            c.set_block_constraints(2, 9)
        assert e.value.code == SPK_ERR_ARG and "at least 3 x 3" in str(e.value)
        assert c.sizes()["m"] == 0 and np.array_equal(c.mult(_x(36)), y0)


OPTS = "-ksp_type fgmres -ksp_rtol 1e-8 -pc_type fieldsplit -pc_fieldsplit_type schur -pc_fieldsplit_schur_fact_type full"


@pytest.mark.parametrize("grid", [(33, 17), (9, 5, 7)])
def test_facade_set_operators_constrained(grid):
    three = len(grid) == 3
    B, g = (S.AssembleOperator_Constraints3D if three else S.AssembleOperator_Constraints)(*grid)
    res = []
    for device in (False, True):
        with S.KSP(0) as ksp:
            rhs = (ksp.setOperatorsLaplace3D if three else ksp.setOperatorsLaplace)(*grid, B="device" if device else B)
            if not device:
                rhs = np.concatenate([rhs, g])
            ksp.setFromOptions(OPTS)
            x = ksp.solve(rhs)
            res.append((rhs.tobytes(), ksp.getIterationNumber(), ksp.getConvergedReason(), ksp.getConvergenceHistory().tobytes(),
                        x.tobytes()))
    assert res[0] == res[1] and res[0][2] > 0


def test_runner_constraints_device_prints_what_host_prints():
    exe = os.path.join(ROOT, "saddle_point_petsc_amd", "saddle_point_run")
    args = ["-da_grid_x", "33", "-da_grid_y", "33", "-spk_assembly", "device"] + OPTS.split() + ["-ksp_monitor", "-ksp_converged_reason",
                                                                                                "-solution_view"]
    runs = []
    for route in ("host", "device"):
        cwd = tempfile.mkdtemp()
        out = subprocess.run(["timeout", "-k", "10", "60", exe] + args + ["-spk_constraints", route], capture_output=True, text=True,
                             cwd=cwd)
        assert out.returncode == 0, out.stdout + out.stderr     # (the second child starts only behind a clean first)
        with open(os.path.join(cwd, "test.vtk"), "rb") as fh:
            vtk = fh.read()
        lines = [ln.split(", solve ")[0] for ln in out.stdout.splitlines()]   # (the wall time of the solve aside)
        assert sum("KSP Residual norm" in ln for ln in lines) > 2 and len(lines) > 2 * 33 * 33
        runs.append((lines, vtk))
    assert runs[0] == runs[1]
    view = subprocess.run(["timeout", "-k", "10", "60", exe] + args + ["-spk_constraints", "device", "-ksp_view", "-no_vtk"],
                          capture_output=True, text=True, cwd=tempfile.mkdtemp())
    assert view.returncode == 0 and "A10: written on the device" in view.stdout, view.stdout + view.stderr
