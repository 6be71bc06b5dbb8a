"""The A block and right-hand side of the 3-D generator assembled on the device (spk_set_block_laplace3d,
spk_k_assembly3d.hip) against the host assembler: the slab bit for bit through the test hook, the context it leaves
against the context the host arrays leave (sizes, layout, diagonal, products, residual histories: same operator bits,
same kernels), the multigrid refresh over it, its refusals, logical ranks and the KSP facade.

Grids: those of the CPU file (2 x 2 x 2 up to 5 x 4 x 3: corners, one element, odd and non-cubic) plus 37 x 3 x 3, 3 x 37 x 3
and 3 x 3 x 37 -- 37 nodes in a line cross the kernel's 4-node strip nine times with a 1-node tail, and 37 lines or planes
take the workgroup index through every (j, k); slabs: the CPU file's plus planes [1, 3) of the grids with mz >= 4, both of
whose neighbouring element layers belong to other ranks."""
import functools
import threading

import numpy as np
import pytest

import saddle_point_petsc_amd as S
from test_assembly3d_cpu import GRIDS as CPU_GRIDS, slabs as cpu_slabs, random_kappa

pytestmark = pytest.mark.gpu
GRIDS = CPU_GRIDS + [(37, 3, 3), (3, 37, 3), (3, 3, 37)]
SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6


def slabs(mx, my, mz):
    out = list(cpu_slabs(mx, my, mz))
    if mz >= 4:
        out.append((3 * mx * my, 3 * mx * my * 3))
    return out


def smooth_kappa(mx, my, mz):
    z, y, x = np.meshgrid((np.arange(mz - 1) + 0.5) / (mz - 1), (np.arange(my - 1) + 0.5) / (my - 1),
                          (np.arange(mx - 1) + 0.5) / (mx - 1), indexing="ij")
    return 1.0 + 0.5 * np.sin(2.0 * x) * np.cos(3.0 * y) * np.cos(1.5 * z)


@functools.lru_cache(maxsize=None)
def host(mx, my, mz, rb, re, apply_bc, kind):
    """the host assembler's slab, computed once per case"""
    kappa = {"none": None, "random": random_kappa(mx, my, mz), "two": np.full((mz - 1, my - 1, mx - 1), 2.0),
             "smooth": smooth_kappa(mx, my, mz)}[kind]
    return S.AssembleOperator_Laplace3D(mx, my, mz, rb, re, apply_bc=bool(apply_bc), nthreads=4, kappa=kappa), kappa


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


def same_slab(got, want):
    (A, f), (A0, f0) = got, want
    assert np.array_equal(A.rowptr, A0.rowptr) and A.rowptr.tobytes() == A0.rowptr.tobytes()
    assert np.array_equal(A.colidx, A0.colidx) and A.colidx.tobytes() == A0.colidx.tobytes()
    assert np.array_equal(A.val, A0.val) and A.val.tobytes() == A0.val.tobytes()
    assert np.array_equal(f, f0) and f.tobytes() == f0.tobytes()


@pytest.mark.parametrize("apply_bc", [0, 1])
@pytest.mark.parametrize("mx,my,mz", GRIDS)
def test_kernel_slab_is_the_host_slab(ctx, mx, my, mz, apply_bc):
    n = 3 * mx * my * mz
    kdev = ctx.vec_create(random_kappa(mx, my, mz).reshape(-1))
    try:
        for rb, re in slabs(mx, my, mz):
            want, _ = host(mx, my, mz, rb, re, apply_bc, "none")
            same_slab(ctx.assemble_laplace3d_csr(mx, my, mz, rb, re, apply_bc=apply_bc), want)
            want, kappa = host(mx, my, mz, rb, re, apply_bc, "random")
            same_slab(ctx.assemble_laplace3d_csr(mx, my, mz, rb, re, kappa=kappa, apply_bc=apply_bc), want)   # a host array
            same_slab(ctx.assemble_laplace3d_csr(mx, my, mz, rb, re, kappa=kdev, apply_bc=apply_bc), want)    # a device vector
            assert want[0].ncols == n
    finally:
        ctx.vec_destroy(kdev)


def _x(n):
    return np.sin(0.37 * np.arange(n))


def _pair(grid, kind):
    """two contexts with the same A00: from the host arrays, and assembled on the device; the device route's f"""
    mx, my, mz = grid
    (A, f), kappa = host(mx, my, mz, 0, 3 * mx * my * mz, 1, kind)
    ch, cd = S.Context(0), S.Context(0)
    ch.set_block(S.BLOCK_A00, A)
    fd = cd.set_block_laplace3d(mx, my, mz, kappa=kappa, rhs=True)
    assert fd.tobytes() == f.tobytes()
    assert cd.assembly_seconds() > 0.0 and ch.assembly_seconds() == 0.0
    return ch, cd, f


@pytest.mark.parametrize("kind", ["none", "random"])
@pytest.mark.parametrize("grid", [(9, 9, 11), (17, 15, 13)])
def test_context_equals_the_host_fed_context(grid, kind):
    ch, cd, f = _pair(grid, kind)
    try:
        assert cd.sizes() == ch.sizes()
        assert cd.spmv_info() == ch.spmv_info()
        n = ch.sizes()["n_local"]
        assert cd.mult(_x(n)).tobytes() == ch.mult(_x(n)).tobytes()
        B, g = S.AssembleOperator_Constraints3D(*grid)
        hist = []
        for c in (ch, cd):
            c.set_block(S.BLOCK_A10, B)
            c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL)
            hist.append((c.jacobi_diag().tobytes(), c.fgmres(np.concatenate([f, g]), rtol=1e-10)[1]))
        assert hist[0][0] == hist[1][0]
        assert hist[0][1]["its"] == hist[1][1]["its"] and hist[0][1]["reason"] == hist[1][1]["reason"] and hist[0][1]["reason"] > 0
        assert hist[0][1]["history"].tobytes() == hist[1][1]["history"].tobytes()
        assert cd.mult(_x(n + 6)).tobytes() == ch.mult(_x(n + 6)).tobytes()
    finally:
        ch.close()
        cd.close()


def test_refresh_over_the_device_assembled_operator():
    grid = (9, 9, 11)
    amg = dict(setup="device")
    its = {}
    with S.Context(0) as cd, S.Context(0) as ch:
        for step, kind in enumerate(["none", "two", "smooth"]):
            (A, f), kappa = host(*grid, 0, 3 * 9 * 9 * 11, 1, kind)
            cd.set_block_laplace3d(*grid, kappa=kappa)
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
    grid = (9, 9, 11)
    with S.Context(0) as c:
        c.set_block_laplace3d(*grid)
        n = c.sizes()["n_local"]
        y0 = c.mult(_x(n))
        bad = random_kappa(*grid)
        bad[3, 5, 2] = 0.0
        kdev = c.vec_create(bad.reshape(-1))
        for kappa in (bad, kdev):                                  # a host array, a device vector
            with pytest.raises(S.SpkError) as e:
                c.set_block_laplace3d(*grid, kappa=kappa)
            assert e.value.code == SPK_ERR_ARG
            assert c.mult(_x(n)).tobytes() == y0.tobytes()
        c.vec_destroy(kdev)
        with pytest.raises(S.SpkError) as e:
            c.set_block_laplace3d(2000, 2000, 2000)                # 2.4e10 rows: refused before anything is allocated
        assert e.value.code == SPK_ERR_UNSUPPORTED
        assert c.sizes()["n_local"] == n and c.mult(_x(n)).tobytes() == y0.tobytes()
        for side in ((1, 9, 11), (9, 1, 11), (9, 9, 1)):
            with pytest.raises(S.SpkError) as e:
                c.set_block_laplace3d(*side)
            assert e.value.code == SPK_ERR_ARG
        assert c.sizes()["n_local"] == n and c.mult(_x(n)).tobytes() == y0.tobytes()


def _group_mult(P, grid, device):
    grp = S.LocalGroup(P)
    out, errs = [None] * P, []
    mx, my, mz = grid

    def work(r):
        try:
            b, e = S.partition_slab3d(mx, my, mz, r, P)
            with S.Context(0) as c:
                c.comm_init_local(grp, r)
                if device:
                    c.set_block_laplace3d(mx, my, mz)
                else:
                    c.set_block(S.BLOCK_A00, host(mx, my, mz, b, e, 1, "none")[0][0])
                out[r] = (b, e, c.mult(_x(3 * mx * my * mz)[b:e]))
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
    grid = (9, 9, 11)
    dev, hst = _group_mult(P, grid, True), _group_mult(P, grid, False)
    for (b, e, y), (b0, e0, y0) in zip(dev, hst):
        assert (b, e) == (b0, e0) and y.tobytes() == y0.tobytes()


OPTS = "-ksp_type fgmres -ksp_rtol 1e-8 -pc_type fieldsplit -pc_fieldsplit_type schur -pc_fieldsplit_schur_fact_type full"


def test_facade_set_operators_laplace3d():
    grid = (9, 9, 11)
    (A, f), _ = host(*grid, 0, 3 * 9 * 9 * 11, 1, "none")
    B, g = S.AssembleOperator_Constraints3D(*grid)
    res = []
    for device in (False, True):
        with S.KSP(0) as ksp:
            if device:
                fd = ksp.setOperatorsLaplace3D(*grid, B=B)
                assert fd.tobytes() == f.tobytes()
            else:
                ksp.setOperators(A, B)
            ksp.setFromOptions(OPTS)
            x = ksp.solve(np.concatenate([f, g]))
            res.append((ksp.getIterationNumber(), ksp.getConvergedReason(), ksp.getConvergenceHistory().tobytes(), x.tobytes()))
    assert res[0] == res[1] and res[0][1] > 0
