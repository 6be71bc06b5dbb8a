"""-pc_type mg on variable-coefficient operators, host route (no GPU): the fields of tests/_mg_fields.py.

1. Every field discriminates: the numpy V-cycle (test_mg_sides_cpu.vcycle_ref) restated with one deliberate mis-indexing
   moves the result by at least 1e-6 relative in each coefficient region -- and on the constant-coefficient operator the
   first two move it by less than 1e-12, which is the gap the fields close.
2. The host Galerkin values of both routes against scipy's P^T A_l P on the new operators, `skew` included.
3. The float64 numpy V-cycle against a numpy.longdouble restatement: the reference's own error, which the 1e-12 bar of
   test_gpu_mg_varcoef.py stands on.
(The non-symmetric value rule of tests/host/galerkin_stencil_check.cpp runs with test_mg_galerkin_cpu.py's sanitizer build.)"""
import numpy as np
import pytest
import scipy.sparse as sp

import _mg_fields as F
import saddle_point_petsc_amd as S
import test_mg_galerkin_cpu as G
from test_mg_sides_cpu import vcycle_ref

U = 2.0 ** -53


# ---- the V-cycle once more, with D^-1 as an argument and in any precision -----------------------------------------------
def vcycle_with(A, P, Ci, lam, b, dinv=None, dtype=np.float64, smooth_its=2, esteig=(0, 0.1, 0, 1.1)):
    """vcycle_ref's operations in its order.  dinv: a list per level in place of 1 / diag(A_l).  dtype numpy.longdouble: every
    operand widened first (the operators as dense copies), every operation in that precision."""
    L = len(A)
    wide = dtype is not np.float64
    if wide:
        A = [a.toarray().astype(dtype) for a in A]
        P = [p.toarray().astype(dtype) for p in P]
        Ci = Ci.astype(dtype)
        diag = [np.diagonal(a) for a in A]
    else:
        diag = [a.diagonal() for a in A]
    if dinv is None:
        dinv = [dtype(1.0) / np.where(d == 0.0, dtype(1.0), d) for d in diag]
    coef = []
    for l in range(L - 1):
        lo, hi = dtype(esteig[1]) * dtype(lam[l]), dtype(esteig[3]) * dtype(lam[l])
        th, de = dtype(0.5) * (hi + lo), dtype(0.5) * (hi - lo)
        sg = th / de
        rho = dtype(1.0) / sg
        al, be = [dtype(1.0) / th], [dtype(0.0)]
        for _ in range(1, smooth_its):
            rn = dtype(1.0) / (dtype(2.0) * sg - rho)
            al.append(dtype(2.0) * rn / de)
            be.append(rn * rho)
            rho = rn
        coef.append((al, be))

    def smooth(l, bb, y):
        prev = None
        for al, be in zip(*coef[l]):
            if y is None:
                yn = al * (dinv[l] * bb)
            else:
                yn = y + al * (dinv[l] * (bb - A[l] @ y))
                if be != 0.0:
                    yn = yn + be * (y - (prev if prev is not None else dtype(0.0)))
            prev, y = y, yn
        return y

    def rec(l, bb):
        if l == L - 1:
            return Ci @ bb
        y = smooth(l, bb, None)
        e = rec(l + 1, P[l].T @ (bb - A[l] @ y))
        return smooth(l, bb, y + P[l] @ e)

    return rec(0, np.asarray(b, dtype))


# ---- the three mis-indexings, all on level 1 (the first level the stencil operator and the fused tail cover) ------------
def _dinv(A):
    return [1.0 / np.where(a.diagonal() == 0.0, 1.0, a.diagonal()) for a in A]


def dinv_of_the_other_component(A, dims, bs, inner=False):
    """level 1 reads D^-1 of the next component of the same node (cyclically); bs 1: of the previous node in x.  inner: only
    at the nodes off the level's edge"""
    d = _dinv(A)
    nx, ny, nz = dims[1]
    wrong = np.roll(d[1].reshape(-1, bs), 1, axis=1) if bs > 1 else np.roll(d[1].reshape(-1, nx), 1, axis=1).reshape(-1, 1)
    n = np.arange(nx * ny * nz)
    i, j, k = n % nx, n // nx % ny, n // (nx * ny)
    edge = (i == 0) | (i == nx - 1) | (j == 0) | (j == ny - 1) | ((nz > 1) & ((k == 0) | (k == nz - 1)))
    d[1] = np.where((edge & inner)[:, None], d[1].reshape(-1, bs), wrong).ravel()
    return d


def dinv_of_the_previous_node(A, dims, bs):
    """level 1 reads D^-1 of the same component one node back in x, at the x-interior nodes"""
    d = _dinv(A)
    d1 = d[1].reshape(-1, bs).copy()
    nodes = np.array(x_interior_nodes(dims[1]))
    d1[nodes] = d[1].reshape(-1, bs)[nodes - 1]
    d[1] = d1.ravel()
    return d


def x_interior_nodes(d):
    """nodes whose row and whose previous node's row are translates of one another on a constant-coefficient operator: both
    at least two nodes from either end in x (a coarse basis function next to the end node couples to it)"""
    nx = d[0]
    return [n for n in range(d[0] * d[1] * d[2]) if 3 <= n % nx <= nx - 3]


def rows_of_the_previous_node(A1, d, bs):
    """every x-interior row of level 1 holds the stored values of the same component's row one node back in x"""
    A1 = A1.tocsr()
    rp, v = A1.indptr, A1.data.copy()
    nodes = x_interior_nodes(d)
    assert len(nodes) >= 2
    for n in nodes:
        for a in range(bs):
            r, q = n * bs + a, (n - 1) * bs + a
            assert rp[r + 1] - rp[r] == rp[q + 1] - rp[q]
            v[rp[r]:rp[r + 1]] = A1.data[rp[q]:rp[q + 1]]
    return sp.csr_matrix((v, A1.indices.copy(), rp.copy()), shape=A1.shape)


def transposed_blocks(A1, d, bs):
    """every off-diagonal bs x bs block of level 1 transposed.  bs 1, where a block is one number: every row not on the
    grid's edge reads the mirrored stencil slot, A[r, r + o] <- A[r, r - o]"""
    D = A1.toarray()
    n = D.shape[0]
    if bs > 1:
        N = n // bs
        B = D.reshape(N, bs, N, bs)
        T = B.transpose(0, 3, 2, 1).copy()
        for I in range(N):
            T[I, :, I, :] = B[I, :, I, :]
        out = T.reshape(n, n)
    else:
        out = D.copy()
        for r in range(n):
            i, j = r % d[0], r // d[0]
            if 1 <= i <= d[0] - 2 and 1 <= j <= d[1] - 2:
                for o in range(1, d[0] + 2):
                    out[r, r + o], out[r, r - o] = D[r, r - o], D[r, r + o]
    out = sp.csr_matrix(out)
    assert (out != 0).nnz == (A1 != 0).nnz
    return out


def _moves(shape, field):
    """the per-region distance of each mis-indexed V-cycle from the right one"""
    _, bs, _ = F.SHAPES[shape]
    info, (A, P, Ci) = F.host_hierarchy(shape, field)
    lam, dims = info["lambda_max"], info["dims"]
    assert info["levels"] >= 3
    b = F.rhs(A[0].shape[0])
    ref = vcycle_ref(A, P, Ci, lam, b)
    assert vcycle_with(A, P, Ci, lam, b).tobytes() == ref.tobytes()   # the restatement is the reference
    reg = F.regions(shape)
    out = {}
    for key, wrong in (("dinv", dinv_of_the_other_component(A, dims, bs)), ("dinv-inner", dinv_of_the_other_component(A, dims, bs, True)),
                       ("dinv-x", dinv_of_the_previous_node(A, dims, bs))):
        out[key] = F.region_rel(vcycle_with(A, P, Ci, lam, b, dinv=wrong), ref, reg)
    for key, wrong in (("row", rows_of_the_previous_node), ("block", transposed_blocks)):
        B = list(A)
        B[1] = wrong(A[1], dims[1], bs)
        out[key] = F.region_rel(vcycle_with(B, P, Ci, lam, b, dinv=_dinv(A)), ref, reg)
    return out


def _show(shape, field, m):
    print(f"{shape} {field}: moved per region (soft, stiff) by " + ", ".join(f"{k} {v[0]:.2e} {v[1]:.2e}" for k, v in m.items()))


# ---- 1. every field discriminates --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,field", F.cases())
def test_every_field_discriminates(shape, field):
    """Each mis-indexing on level 1 moves one V-cycle by at least 1e-6 relative in each region: D^-1 of the other component
    (bs 1: of the previous node in x) at every node, D^-1 of the previous node
    at the x-interior nodes, the previous node's rows, the transposed blocks (bs 1: the mirrored slot).  Smallest values
    measured, all under `jump` in the stiff half: D^-1 of the other component 4.1e-6 (33x33), D^-1 of the previous node 2.8e-6,
    its rows 1.1e-5, the transposed blocks 1.5e-5 (17x9x5)."""
    m = _moves(shape, field)
    _show(shape, field, m)
    for k in ("dinv", "dinv-x", "row", "block"):   # dinv-inner is printed: the record of what `jump` alone leaves blind
        assert min(m[k]) >= 1e-6, (shape, field, k, m[k])


@pytest.mark.parametrize("shape", list(F.SHAPES))
def test_the_constant_operator_does_not(shape):
    """The gap: on the constant-coefficient operator a kernel that reads D^-1 or the rows of the previous node in x moves one
    V-cycle by less than 1e-12 -- under the bar of every toleranced check (measured: at most 3.7e-16).  D^-1 of the other
    component is as blind a spot only where the components see the same grid: off the level's edge (the Dirichlet sides of
    the components differ: 3 against 2.5 next to the edge of 33 x 33's level 1) on a grid with hx = hy, which of the shapes
    here is 33 x 33 alone; there it moves nothing at all.  At every node it moves the constant operator's V-cycle by 1.1e-3
    (33x33) to 1.9e-2 (65x33), so that one was never blind; the values are printed."""
    m = _moves(shape, "const")
    _show(shape, "const", m)
    assert max(m["row"]) < 1e-12 and max(m["dinv-x"]) < 1e-12, m
    if shape == "33x33":
        assert max(m["dinv-inner"]) < 1e-12, m


# ---- 2. the host Galerkin values against scipy -------------------------------------------------------------------------
@pytest.mark.parametrize("shape,field", F.cases(skew=True))
def test_stencil_values_against_scipy_and_bitwise_symmetry(shape, field, monkeypatch):
    """test_mg_galerkin_cpu's check on the new operators: its derived bound 2 9^d 2^-53 T entrywise, and bitwise symmetry.
    Under `skew` A_0 is not symmetric and the symmetrisation averages numbers that differ in the second digit."""
    grid, bs, sides = F.SHAPES[shape]
    A = F.operator(shape, field)
    if field == "skew":
        M = F.to_sp((A.rowptr, A.colidx, A.val, (A.nrows, A.nrows)))
        asym = abs(M - M.T).max() / abs(M).max()
        print(f"{shape} skew: |A_0 - A_0^T| / |A_0| = {asym:.2e}")
        assert asym >= 1e-3
    key = f"{shape}/{field}"
    monkeypatch.setitem(G.SHAPES, key, (grid, bs, sides, None))
    h = S.AmgHierarchy(A, **F.amg_kw(shape, galerkin="stencil"))
    try:
        assert np.all(np.isfinite(h.info()["lambda_max"][:-1]))
        G.test_values_against_scipy_level_by_level_and_bitwise_symmetry((key, h, None))
    finally:
        h.close()


@pytest.mark.parametrize("shape,field", F.cases(skew=True))
def test_products_values_against_scipy(shape, field):
    """The products route to the bar test_mg_grid_cpu and test_mg_sides_cpu hold it to: 1e-13 of the norm of (G + G^T) / 2,
    and a symmetric result.  The entrywise ratio to the stencil route's bound is printed: under `jump` the norm is the
    stiff half's."""
    grid = F.SHAPES[shape][0]
    d = 3 if grid[2] > 1 else 2
    info, (A, P, _) = F.host_hierarchy(shape, field, "products")
    worst_n = worst_e = 0.0
    for l in range(info["levels"] - 1):
        Gm = (P[l].T @ A[l] @ P[l]).toarray()
        ref = 0.5 * (Gm + Gm.T)
        N = A[l + 1].toarray()
        T = (abs(P[l]).T @ abs(A[l]) @ abs(P[l])).toarray()
        bound = 2.0 * 9 ** d * U * 0.5 * (T + T.T)
        err = np.abs(N - ref)
        worst_n = max(worst_n, float(np.linalg.norm(N - ref) / np.linalg.norm(ref)))
        worst_e = max(worst_e, float((err[bound > 0] / bound[bound > 0]).max()))
        assert np.linalg.norm(N - ref) <= 1e-13 * np.linalg.norm(ref), (shape, field, l)
        assert (A[l + 1] != A[l + 1].T).nnz == 0 and np.all(N[bound == 0] == 0.0)
    print(f"{shape} {field} products: largest |A_l+1 - ref| / |ref| = {worst_n:.2e}, largest entrywise |A_l+1 - ref| / bound = {worst_e:.4f}")


# ---- 3. the reference alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("galerkin", ["stencil", "products"])
@pytest.mark.parametrize("field", ("const",) + F.KAPPA_FIELDS)
def test_reference_against_longdouble(field, galerkin):
    """The float64 vcycle_ref against the same operations in numpy.longdouble (64-bit significand) on dense copies of the
    33 x 33 hierarchy: at most 1e-14 in each region.  Measured: at most 3.7e-16 (jump, stiff half); 2.4e-16 on the constant
    operator.  The GPU file's 1e-12 bar has two decades over this."""
    assert np.finfo(np.longdouble).nmant >= 63
    info, (A, P, Ci) = F.host_hierarchy("33x33", field, galerkin)
    b = F.rhs(A[0].shape[0])
    ref = vcycle_ref(A, P, Ci, info["lambda_max"], b)
    wide = vcycle_with(A, P, Ci, info["lambda_max"], b, dtype=np.longdouble)
    reg = F.regions("33x33")
    dist = [float(np.linalg.norm((ref - wide)[reg == r]) / np.linalg.norm(wide[reg == r])) for r in (0, 1)]
    print(f"33x33 {field} {galerkin}: float64 V-cycle {dist[0]:.2e} (soft) {dist[1]:.2e} (stiff) off longdouble")
    assert max(dist) <= 1e-14
