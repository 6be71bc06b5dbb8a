"""The coefficient kappa of the host assembler (SpkAssembleOperator_LaplaceKappa) and the row-pointer helper the host
and the device route share.  No GPU: the host twin is the CPU oracle of the device assembly kernel (test_gpu_assembly.py)."""
import ctypes as C

import numpy as np
import pytest

import saddle_point_petsc_amd as spk
from saddle_point_petsc_amd._lib import lib

GRIDS = [(2, 2), (3, 3), (5, 4), (4, 5), (33, 17)]
SPK_ERR_ARG = -1


def slabs(mx, my):
    """(row_begin, row_end): the whole grid, the first line, the last line, and lines [5,11) of (33,17)."""
    line = 2 * mx
    out = [(0, line * my), (0, line), (line * (my - 1), line * my)]
    if (mx, my) == (33, 17):
        out.append((5 * line, 11 * line))
    return out


def random_kappa(mx, my, seed=20240607):
    return np.random.default_rng(seed).uniform(0.5, 2.0, (my - 1, mx - 1))


def coord(i, m):
    return 0.0 + (1.0 / float(m - 1)) * float(i)


def corner(oi, oj):
    return (0 if oj == 0 else 1) if oi == 0 else (3 if oj == 0 else 2)


def numpy_gather(mx, my, rb, re, kappa, apply_bc):
    """The slab's values entry by entry: the sum, from 0.0, over the elements that hold both nodes in ascending (ej, ei)
    of FormStressOperatorQ12D(xe, [kappa_e] * 4)."""
    Ke = {}
    for ej in range(my - 1):
        for ei in range(mx - 1):
            xe = [coord(ei, mx), coord(ej, my), coord(ei, mx), coord(ej + 1, my),
                  coord(ei + 1, mx), coord(ej + 1, my), coord(ei + 1, mx), coord(ej, my)]
            Ke[ej, ei] = spk.FormStressOperatorQ12D(xe, [kappa[ej, ei]] * 4)
    bnd = lambda i, j: i == 0 or i == mx - 1 or j == 0 or j == my - 1  # noqa: E731
    cols, vals, rowptr = [], [], [0]
    for j in range(rb // (2 * mx), re // (2 * mx)):
        for i in range(mx):
            for c in range(2):
                grow = (j * mx + i) * 2 + c
                for cj in range(max(j - 1, 0), min(j + 1, my - 1) + 1):
                    for ci in range(max(i - 1, 0), min(i + 1, mx - 1) + 1):
                        for d in range(2):
                            gcol = (cj * mx + ci) * 2 + d
                            v = np.float64(0.0)
                            for ej in range(max(j, cj) - 1, min(j, cj) + 1):
                                for ei in range(max(i, ci) - 1, min(i, ci) + 1):
                                    if 0 <= ej <= my - 2 and 0 <= ei <= mx - 2:
                                        v = v + Ke[ej, ei][corner(i - ei, j - ej) * 2 + c, corner(ci - ei, cj - ej) * 2 + d]
                            if apply_bc and (bnd(i, j) or bnd(ci, cj)):
                                v = 1.0 if gcol == grow else 0.0
                            cols.append(gcol)
                            vals.append(v)
                rowptr.append(len(cols))
    return np.array(rowptr, np.int32), np.array(cols, np.int32), np.array(vals)


def same(A, f, A0, f0):
    assert A.rowptr.tobytes() == A0.rowptr.tobytes() and A.colidx.tobytes() == A0.colidx.tobytes()
    assert A.val.tobytes() == A0.val.tobytes() and f.tobytes() == f0.tobytes()


@pytest.mark.parametrize("mx,my", GRIDS)
@pytest.mark.parametrize("apply_bc", [0, 1])
def test_kappa_null_and_ones_are_the_existing_assembler(mx, my, apply_bc):
    for rb, re in slabs(mx, my):
        A0, f0 = spk.AssembleOperator_Laplace(mx, my, rb, re, apply_bc=apply_bc, nthreads=2)
        nnz = A0.nnz
        # NULL, through the new entry point itself
        rowptr, colidx, val, f = np.zeros(re - rb + 1, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz), np.zeros(re - rb)
        assert lib.SpkAssembleOperator_LaplaceKappa(mx, my, rb, re, None, rowptr, colidx, val, f.ctypes.data, apply_bc, 2) == 0
        same(spk.CSR(rowptr, colidx, val, A0.ncols, rb), f, A0, f0)
        A1, f1 = spk.AssembleOperator_Laplace(mx, my, rb, re, apply_bc=apply_bc, nthreads=3, kappa=np.ones((my - 1, mx - 1)))
        same(A1, f1, A0, f0)


@pytest.mark.parametrize("mx,my", GRIDS)
def test_kappa_two_doubles_every_free_value(mx, my):
    two = np.full((my - 1, mx - 1), 2.0)
    for rb, re in slabs(mx, my):
        for apply_bc in (0, 1):
            A0, f0 = spk.AssembleOperator_Laplace(mx, my, rb, re, apply_bc=apply_bc)
            A2, f2 = spk.AssembleOperator_Laplace(mx, my, rb, re, apply_bc=apply_bc, kappa=two)
            assert np.array_equal(A2.rowptr, A0.rowptr) and np.array_equal(A2.colidx, A0.colidx)
            assert f2.tobytes() == f0.tobytes()          # f does not depend on kappa
            rows = np.repeat(np.arange(rb, re), np.diff(A0.rowptr))
            node = lambda g: ((g // 2) % mx, (g // 2) // mx)  # noqa: E731
            onb = lambda g: (node(g)[0] == 0) | (node(g)[0] == mx - 1) | (node(g)[1] == 0) | (node(g)[1] == my - 1)  # noqa: E731
            dirichlet = (onb(rows) | onb(A0.colidx.astype(np.int64))) if apply_bc else np.zeros(A0.nnz, bool)
            assert np.array_equal(A2.val[~dirichlet], 2.0 * A0.val[~dirichlet])
            ident = (rows == A0.colidx).astype(np.float64)
            assert np.array_equal(A2.val[dirichlet], ident[dirichlet])     # Dirichlet rows and columns stay identity


@pytest.mark.parametrize("mx,my", GRIDS)
@pytest.mark.parametrize("apply_bc", [0, 1])
def test_random_kappa_against_a_numpy_gather(mx, my, apply_bc):
    kappa = random_kappa(mx, my)
    for rb, re in slabs(mx, my):
        A, f = spk.AssembleOperator_Laplace(mx, my, rb, re, apply_bc=apply_bc, nthreads=2, kappa=kappa)
        rowptr, cols, vals = numpy_gather(mx, my, rb, re, kappa, apply_bc)
        assert np.array_equal(A.rowptr, rowptr) and np.array_equal(A.colidx, cols)
        assert A.val.tobytes() == vals.tobytes()
        _, f0 = spk.AssembleOperator_Laplace(mx, my, rb, re, apply_bc=apply_bc)
        assert f.tobytes() == f0.tobytes()


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_bad_kappa_is_refused_and_writes_nothing(bad):
    mx, my = 5, 4
    kappa = random_kappa(mx, my).reshape(-1)
    kappa[7] = bad
    n, nnz = spk.grid_sizes(mx, my)
    rowptr, colidx = np.full(n + 1, -7, np.int32), np.full(nnz, -7, np.int32)
    val, f = np.full(nnz, -7.0), np.full(n, -7.0)
    rc = lib.SpkAssembleOperator_LaplaceKappa(mx, my, 0, n, kappa.ctypes.data, rowptr, colidx, val, f.ctypes.data, 1, 2)
    assert rc == SPK_ERR_ARG
    assert (rowptr == -7).all() and (colidx == -7).all() and (val == -7.0).all() and (f == -7.0).all()
    assert lib.SpkAssemblyCheckKappa(mx, my, kappa.ctypes.data) == SPK_ERR_ARG
    with pytest.raises(spk.SpkError) as e:
        spk.AssembleOperator_Laplace(mx, my, kappa=kappa)
    assert e.value.code == SPK_ERR_ARG


@pytest.mark.parametrize("mx,my", GRIDS)
def test_shared_row_pointers_equal_the_assembler(mx, my):
    for rb, re in slabs(mx, my):
        A0, _ = spk.AssembleOperator_Laplace(mx, my, rb, re)
        assert np.array_equal(spk.slab_row_pointers(mx, my, rb, re), A0.rowptr)
        assert A0.rowptr[-1] == lib.SpkAssemblySlabNnz(mx, my, rb, re)
