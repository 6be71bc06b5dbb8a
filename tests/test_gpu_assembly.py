"""The A block and right-hand side assembled on the device (spk_set_block_laplace, spk_k_assembly.hip) against the host
assembler: the slab bit for bit through the test hook, the context it leaves against the context the host arrays
leave (sizes, layout, diagonal, products, residual histories: same operator bits, same kernels), the multigrid
refresh over it, its refusals, logical ranks, the KSP facade and the runner.

Grids: those of the CPU file (2 x 2 up to 33 x 17: corners, one element, odd and non-square) plus 300 x 7 and 7 x 300
-- 300 nodes in a line cross the kernel's 32-node strip nine times with a 12-node tail, 7 lines are first, interior
and last; slabs: the CPU file's plus one interior line, both of whose element lines belong to other ranks."""
import functools
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import saddle_point_petsc_amd as S
from test_assembly_kappa_cpu import GRIDS as CPU_GRIDS, slabs as cpu_slabs, random_kappa

pytestmark = pytest.mark.gpu
GRIDS = CPU_GRIDS + [(300, 7), (7, 300)]
SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def slabs(mx, my):
    out = list(cpu_slabs(mx, my))
    if my >= 3:
        out.append((2 * mx * (my // 2), 2 * mx * (my // 2 + 1)))
    return out


def smooth_kappa(mx, my):
    x, y = np.meshgrid((np.arange(mx - 1) + 0.5) / (mx - 1), (np.arange(my - 1) + 0.5) / (my - 1))
    return 1.0 + 0.5 * np.sin(2.0 * x) * np.cos(3.0 * y)


@functools.lru_cache(maxsize=None)
def host(mx, my, rb, re, apply_bc, kind):
    """the host assembler's slab, computed once per case"""
    kappa = {"none": None, "random": random_kappa(mx, my), "two": np.full((my - 1, mx - 1), 2.0),
             "smooth": smooth_kappa(mx, my)}[kind]
    return S.AssembleOperator_Laplace(mx, my, rb, re, apply_bc=bool(apply_bc), nthreads=4, kappa=kappa), kappa


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def same_slab(got, want):
    (A, f), (A0, f0) = got, want
    assert np.array_equal(A.rowptr, A0.rowptr)
    assert np.array_equal(A.colidx, A0.colidx)
    assert np.array_equal(A.val, A0.val) and A.val.tobytes() == A0.val.tobytes()
    assert np.array_equal(f, f0) and f.tobytes() == f0.tobytes()


@pytest.mark.parametrize("apply_bc", [0, 1])
@pytest.mark.parametrize("mx,my", GRIDS)
def test_kernel_slab_is_the_host_slab(ctx, mx, my, apply_bc):
    n = 2 * mx * my
    kdev = ctx.vec_create(random_kappa(mx, my).reshape(-1))
    try:
        for rb, re in slabs(mx, my):
            want, _ = host(mx, my, rb, re, apply_bc, "none")
            same_slab(ctx.assemble_laplace_csr(mx, my, rb, re, apply_bc=apply_bc), want)
            want, kappa = host(mx, my, rb, re, apply_bc, "random")
            same_slab(ctx.assemble_laplace_csr(mx, my, rb, re, kappa=kappa, apply_bc=apply_bc), want)   # a host array
            same_slab(ctx.assemble_laplace_csr(mx, my, rb, re, kappa=kdev, apply_bc=apply_bc), want)    # a device vector
            assert want[0].ncols == n
    finally:
        ctx.vec_destroy(kdev)


def _x(n):
    return np.sin(0.37 * np.arange(n))


def _pair(mx, my, kind):
    """two contexts with the same A00: from the host arrays, and assembled on the device; the device route's f"""
    (A, f), kappa = host(mx, my, 0, 2 * mx * my, 1, kind)
    ch, cd = S.Context(0), S.Context(0)
    ch.set_block(S.BLOCK_A00, A)
    fd = cd.set_block_laplace(mx, my, kappa=kappa, rhs=True)
    assert fd.tobytes() == f.tobytes()
    assert cd.assembly_seconds() > 0.0 and ch.assembly_seconds() == 0.0
    return ch, cd, f


@pytest.mark.parametrize("kind", ["none", "random"])
@pytest.mark.parametrize("mx,my", [(33, 17), (64, 64)])
def test_context_equals_the_host_fed_context(mx, my, kind):
    ch, cd, f = _pair(mx, my, kind)
    try:
        assert cd.sizes() == ch.sizes()
        assert cd.spmv_info() == ch.spmv_info()          # (a refused row-type layout is refused by both)
        n = ch.sizes()["n_local"]
        assert cd.mult(_x(n)).tobytes() == ch.mult(_x(n)).tobytes()
        B, g = S.AssembleOperator_Constraints(mx, my)
        hist = []
        for c in (ch, cd):
            c.set_block(S.BLOCK_A10, B)
            c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL)
            hist.append((c.jacobi_diag().tobytes(), c.fgmres(np.concatenate([f, g]), rtol=1e-10)[1]))
        assert hist[0][0] == hist[1][0]
        assert hist[0][1]["its"] == hist[1][1]["its"] and hist[0][1]["reason"] == hist[1][1]["reason"] == 2
        assert hist[0][1]["history"].tobytes() == hist[1][1]["history"].tobytes()
        assert cd.mult(_x(n + 4)).tobytes() == ch.mult(_x(n + 4)).tobytes()
    finally:
        ch.close()
        cd.close()


def test_refresh_over_the_device_assembled_operator():
    mx = my = 65
    amg = dict(setup="device")
    its = {}
    with S.Context(0) as cd, S.Context(0) as ch:
        for step, kind in enumerate(["none", "two", "smooth"]):
            (A, f), kappa = host(mx, my, 0, 2 * mx * my, 1, kind)
            cd.set_block_laplace(mx, my, kappa=kappa)
            cd.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
            # the device-assembled pattern compares equal to itself: the second and third set-up refresh
            assert cd.amg_reuse_info()["refreshed"] is (step > 0)
            ch.set_block(S.BLOCK_A00, A)
            ch.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
            a, b = cd.pipecg(f, rtol=1e-8)[1], ch.pipecg(f, rtol=1e-8)[1]
            assert a["reason"] > 0 and a["its"] == b["its"], (kind, a["its"], b["its"])
            its[kind] = a["its"]
    assert all(v > 0 for v in its.values())


def test_refusals_leave_the_previous_operator():
    mx, my = 33, 17
    with S.Context(0) as c:
        c.set_block_laplace(mx, my)
        n = c.sizes()["n_local"]
        y0 = c.mult(_x(n))
        bad = random_kappa(mx, my)
        bad[3, 5] = 0.0
        kdev = c.vec_create(bad.reshape(-1))
        for kappa in (bad, kdev):                                  # a host array, a device vector
            with pytest.raises(S.SpkError) as e:
                c.set_block_laplace(mx, my, kappa=kappa)
            assert e.value.code == SPK_ERR_ARG
            assert c.mult(_x(n)).tobytes() == y0.tobytes()
        c.vec_destroy(kdev)
        with pytest.raises(S.SpkError) as e:
            c.set_block_laplace(40000, 40000)                      # 3.2e9 rows: refused before anything is allocated
        assert e.value.code == SPK_ERR_UNSUPPORTED
        with pytest.raises(S.SpkError) as e:
            c.set_block_laplace(1, 5)
        assert e.value.code == SPK_ERR_ARG
        assert c.sizes()["n_local"] == n and c.mult(_x(n)).tobytes() == y0.tobytes()


def _group_mult(P, mx, my, device):
    grp = S.LocalGroup(P)
    out, errs = [None] * P, []

    def work(r):
        try:
            b, e = S.partition_slab(mx, my, r, P)
            with S.Context(0) as c:
                c.comm_init_local(grp, r)
                if device:
                    c.set_block_laplace(mx, my)
                else:
                    c.set_block(S.BLOCK_A00, host(mx, my, b, e, 1, "none")[0][0])
                out[r] = (b, e, c.mult(_x(2 * mx * my)[b:e]))
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
def test_logical_ranks_match_host_assembled_slabs(P):
    mx, my = 33, 17
    dev, hst = _group_mult(P, mx, my, True), _group_mult(P, mx, my, False)
    for (b, e, y), (b0, e0, y0) in zip(dev, hst):
        assert (b, e) == (b0, e0) and y.tobytes() == y0.tobytes()


OPTS = "-ksp_type fgmres -ksp_rtol 1e-8 -pc_type fieldsplit -pc_fieldsplit_type schur -pc_fieldsplit_schur_fact_type full"


def test_facade_set_operators_laplace():
    mx, my = 33, 17
    (A, f), _ = host(mx, my, 0, 2 * mx * my, 1, "none")
    B, g = S.AssembleOperator_Constraints(mx, my)
    res = []
    for device in (False, True):
        with S.KSP(0) as ksp:
            if device:
                fd = ksp.setOperatorsLaplace(mx, my, B=B)
                assert fd.tobytes() == f.tobytes()
            else:
                ksp.setOperators(A, B)
            ksp.setFromOptions(OPTS)
            x = ksp.solve(np.concatenate([f, g]))
            res.append((ksp.getIterationNumber(), ksp.getConvergedReason(), ksp.getConvergenceHistory().tobytes(), x.tobytes()))
    assert res[0] == res[1] and res[0][1] > 0


def test_runner_device_route_prints_what_the_host_route_prints():
    exe = os.path.join(ROOT, "saddle_point_petsc_amd", "saddle_point_run")
    args = ["-da_grid_x", "65", "-da_grid_y", "65"] + OPTS.split() + ["-ksp_monitor", "-ksp_converged_reason"]
    runs = []
    for extra in ([], ["-spk_assembly", "device"]):
        cwd = tempfile.mkdtemp()
        out = subprocess.run(["timeout", "-k", "10", "60", exe] + args + extra, capture_output=True, text=True, cwd=cwd)
        assert out.returncode == 0, out.stdout + out.stderr     # (the second child starts only behind a clean first)
        with open(os.path.join(cwd, "test.vtk"), "rb") as fh:
            vtk = fh.read()
        keep = [ln for ln in out.stdout.splitlines() if "KSP Residual norm" in ln or "Linear solve" in ln]
        assert len(keep) > 2
        runs.append((keep, vtk))
    assert runs[0] == runs[1]
    view = subprocess.run(["timeout", "-k", "10", "60", exe] + args + ["-spk_assembly", "device", "-ksp_view", "-no_vtk"],
                          capture_output=True, text=True, cwd=tempfile.mkdtemp())
    assert view.returncode == 0 and "assembled on the device" in view.stdout, view.stdout + view.stderr
