"""Variable-coefficient operators for the -pc_type mg tests (a plain helper module): named fields on the package's own
patterns, so that every layout still applies, with the coefficient region of every row.

On the constant-coefficient discretisation the rows of a level are copies of one another up to rounding, and a kernel that
reads a stored value of the neighbouring node, of the other component or of the transposed block passes every toleranced
check.  The fields here make such values differ in the leading digits:

  const      the constant-coefficient operator (the gap's own record: test_mg_varcoef_cpu.py asserts it does not discriminate)
  smooth     kappa = 1 + U(0, 1) per element
  jump       kappa = 1 on the elements of the lower half in x, 1e4 on the rest.  In 3-D the halves are in z and kappa is
             (1 or 1e4) exp(U(-ln 4, ln 4)): with the halves alone every row stays a translate in x of the previous node's
             row, and reading that row moved the V-cycle by 5e-17 (test_mg_varcoef_cpu.py asks for 1e-6; with a factor
             1 + U(0, 1), D^-1 of the previous node still moved the stiff half, whose norm the Dirichlet rows carry, by 6e-7)
  lognormal  kappa = exp(3 N(0, 1)) per element
  dad        five_point only (bs 1, no element field): D A D with d = exp(U(-ln 4, ln 4)) per row, the pattern kept entry
             for entry
  skew       smooth (dad for five_point) with every stored value multiplied by 1 + 0.05 (u - 0.5), u ~ U(0, 1) per entry:
             the same pattern, values no longer symmetric.  The Galerkin product symmetrises, so only level 0 is
             non-symmetric.

Seeds are fixed; every operator is computed once and never changed.  The regions are the halves of `jump` for every field
(region 1: the nodes that touch an element of the stiff half), so that norms taken per region mean the same under each."""
import functools

import numpy as np
import scipy.sparse as sp

import saddle_point_petsc_amd as S
from test_mg_grid_cpu import five_point

# name -> (grid, bs, sides); hierarchies are built with coarse_eq_limit 10
SHAPES = {
    "33x33": ((33, 33, 1), 2, "odd"),       # rows 2178, 578, 162, 50, 18
    "65x33": ((65, 33, 1), 2, "odd"),       # level 1: 1122 rows in workgroups of 192, chunk edges inside grid lines
    "12x10any": ((12, 10, 1), 2, "any"),    # even-side flags
    "17x9x5": ((17, 9, 5), 3, "odd"),       # a node's three rows fall into two workgroups
    "five17x9": ((17, 9, 1), 1, "odd"),     # odd value offsets: the peeled head and tail of the 16-byte staging
}
KAPPA_FIELDS = ("smooth", "jump", "lognormal")
SEEDS = {"smooth": 7, "jump": 0, "lognormal": 13, "dad": 17, "skew": 19, "rhs": 23}


def fields(shape, skew=False):
    """the symmetric fields of a shape, and `skew` behind them on request"""
    f = ("dad",) if shape.startswith("five") else KAPPA_FIELDS
    return f + (("skew",) if skew else ())


def cases(shapes=None, skew=False, only=None):
    """(shape, field) pairs for a parametrisation"""
    return [(s, f) for s in (shapes or SHAPES) for f in fields(s, skew) if only is None or f in only]


def kappa(shape, field):
    """one coefficient per element, in the assembler's element order (x fastest)"""
    grid = SHAPES[shape][0]
    e = [max(m - 1, 1) for m in grid]
    ne = e[0] * e[1] * e[2]
    rng = np.random.default_rng(SEEDS[field])
    if field == "smooth":
        return 1.0 + rng.random(ne)
    if field == "lognormal":
        return np.exp(3.0 * rng.standard_normal(ne))
    assert field == "jump"
    ek, _, ei = np.unravel_index(np.arange(ne), (e[2], e[1], e[0]))
    if grid[2] > 1:   # halves in z alone leave every row a translate in x of the previous node's: the halves, times `dad`'s factor
        return np.where(ek >= e[2] // 2, 1e4, 1.0) * np.exp(rng.uniform(-np.log(4.0), np.log(4.0), ne))
    return np.where(ei >= e[0] // 2, 1e4, 1.0)


def _copy(A, val):
    return S.CSR(A.rowptr.copy(), A.colidx.copy(), np.ascontiguousarray(val, np.float64), A.nrows)


@functools.lru_cache(maxsize=None)
def problem(shape, field):
    """(A, f) of a shape under a field; f is the assembler's right-hand side, a fixed random vector for five_point"""
    grid, bs, _ = SHAPES[shape]
    if field == "skew":
        A, f = problem(shape, fields(shape)[0])
        u = np.random.default_rng(SEEDS["skew"]).random(A.val.size)
        return _copy(A, A.val * (1.0 + 0.05 * (u - 0.5))), f
    if shape.startswith("five"):
        A = five_point(grid[0], grid[1])
        f = np.random.default_rng(SEEDS["rhs"]).standard_normal(A.nrows)
        if field == "const":
            return A, f
        assert field == "dad"
        d = np.exp(np.random.default_rng(SEEDS["dad"]).uniform(-np.log(4.0), np.log(4.0), A.nrows))
        M = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))
        M = (sp.diags(d) @ M @ sp.diags(d)).tocsr()
        M.sort_indices()
        assert np.array_equal(M.indices, A.colidx) and np.array_equal(M.indptr, A.rowptr)
        return _copy(A, M.data), f
    k = None if field == "const" else kappa(shape, field)
    if grid[2] > 1:
        return S.AssembleOperator_Laplace3D(*grid, kappa=k)
    return S.AssembleOperator_Laplace(grid[0], grid[1], kappa=k)


def operator(shape, field):
    return problem(shape, field)[0]


@functools.lru_cache(maxsize=None)
def regions(shape):
    """the region (0 soft, 1 stiff under `jump`) of every row of level 0: a node is stiff when it touches a stiff element"""
    grid, bs, _ = SHAPES[shape]
    k, _, i = np.unravel_index(np.arange(grid[0] * grid[1] * grid[2]), (grid[2], grid[1], grid[0]))
    node = (k >= (grid[2] - 1) // 2) if grid[2] > 1 else (i >= (grid[0] - 1) // 2)
    reg = np.repeat(node.astype(np.int64), bs)
    reg.setflags(write=False)
    return reg


def region_rel(y, ref, reg):
    """||y - ref|| / ||ref|| over each region separately"""
    return [float(np.linalg.norm((y - ref)[reg == r]) / np.linalg.norm(ref[reg == r])) for r in (0, 1)]


def amg_kw(shape, **kw):
    grid, bs, sides = SHAPES[shape]
    return dict(dict(coarsening="grid", grid=grid, sides=sides, block_size=bs, coarse_eq_limit=10), **kw)


def stencil_kw(shape, **kw):
    """amg_kw on the all-stencil route: what precision='single' needs"""
    return amg_kw(shape, **dict(dict(galerkin="stencil", operator="stencil"), **kw))


@functools.lru_cache(maxsize=None)
def host_hierarchy(shape, field, galerkin="stencil"):
    """(info, (A_l, P_l, C^-1)) of the host build, computed once; nobody writes into it"""
    from test_mg_sides_cpu import hierarchy_mats
    h = S.AmgHierarchy(operator(shape, field), **amg_kw(shape, galerkin=galerkin))
    info = h.info()
    mats = hierarchy_mats(h.matrix, info)
    h.close()
    return info, mats


def to_sp(m):
    return sp.csr_matrix((m[2], m[1], m[0]), shape=m[3])


def rhs(n, seed=3):
    return np.random.default_rng(seed).standard_normal(n)
