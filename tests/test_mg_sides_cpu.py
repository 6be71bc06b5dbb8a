"""Grid coarsening on even sides (spk_amg_opts.sides = SPK_AMG_SIDES_ANY, -spk_mg_sides any) without a GPU, through the
host-only builder: the grids of every level against a restatement of the rule, every P against the numpy Kronecker
product byte for byte, `any` on odd grids against `odd`, the option's values, the facade, the refresh, and the iteration
counts of a numpy V-cycle on even grids against the odd grids one node larger.

The rule: a side of m nodes halves to m // 2 + 1 when m >= 4 (`any`) -- (m + 1) / 2 of an odd m; of an even m the coarse
nodes are the fine indices 0, 2, ..., m - 2 and m - 1, and fine m - 1 has the one parent m / 2 with weight 1."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError

SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6


# ---- the rule, restated -------------------------------------------------------------------------------------------------
def coarse_side(m, sides="any"):
    halves = m >= 4 if sides == "any" else m >= 5 and m % 2 == 1
    return m // 2 + 1 if halves else m


def level_dims(d, bs, sides="any", coarse_eq_limit=10, max_levels=10):
    """the node grid of every level: stop at n <= coarse_eq_limit, at max_levels, or when no direction halves"""
    out = [tuple(d)]
    while bs * int(np.prod(out[-1])) > coarse_eq_limit and len(out) < max_levels:
        c = tuple(coarse_side(m, sides) for m in out[-1])
        if c == out[-1]:
            break
        out.append(c)
    return out


def prolong_1d(m, sides="any"):
    """m fine nodes -> coarse_side(m): even i -> i / 2 (weight 1); odd i -> (i - 1) / 2 and (i + 1) / 2 (1/2 each), but the
    last index of an even side -> m / 2 alone (weight 1); a side that does not halve: the identity"""
    mc = coarse_side(m, sides)
    if mc == m:
        return sp.identity(m, format="csr")
    P = np.zeros((m, mc))
    for i in range(m):
        if i % 2 == 0:
            P[i, i // 2] = 1.0
        elif i == m - 1:
            P[i, m // 2] = 1.0
        else:
            P[i, (i - 1) // 2] = P[i, (i + 1) // 2] = 0.5
    return sp.csr_matrix(P)


def prolong_ref(d, bs, sides="any"):
    """P_z (x) P_y (x) P_x (x) I_bs as sorted CSR"""
    P = sp.kron(prolong_1d(d[2], sides), sp.kron(prolong_1d(d[1], sides), sp.kron(prolong_1d(d[0], sides), sp.identity(bs)))).tocsr()
    P.sum_duplicates()
    P.eliminate_zeros()
    P.sort_indices()
    return P


def test_the_restated_rule():
    chain = [66]
    while coarse_side(chain[-1]) != chain[-1]:
        chain.append(coarse_side(chain[-1]))
    assert chain == [66, 34, 18, 10, 6, 4, 3]
    assert [coarse_side(m) for m in (2, 3, 4, 5, 1024, 1025)] == [2, 3, 3, 3, 513, 513]
    assert [coarse_side(m, "odd") for m in (4, 5, 64, 65)] == [4, 3, 64, 33]
    P = prolong_1d(6).toarray()   # 6 -> 4: coarse nodes at fine 0, 2, 4 and 5
    assert np.array_equal(P, np.array([[1, 0, 0, 0], [.5, .5, 0, 0], [0, 1, 0, 0], [0, .5, .5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))
    assert prolong_1d(66).nnz == 3 * 66 // 2 - 1


# ---- 1, 2. the grids and the prolongators of every level ---------------------------------------------------------------------
GRIDS = [((64, 64, 1), 2), ((66, 66, 1), 2), ((64, 48, 1), 2), ((100, 70, 1), 2), ((65, 64, 1), 2), ((6, 6, 1), 2), ((4, 4, 1), 2),
         ((16, 16, 16), 3), ((6, 4, 3), 3), ((4, 5, 6), 3)]
EXPECT_DIMS = {
    (66, 66, 1): [(66, 66, 1), (34, 34, 1), (18, 18, 1), (10, 10, 1), (6, 6, 1), (4, 4, 1), (3, 3, 1)],
    (64, 48, 1): [(64, 48, 1), (33, 25, 1), (17, 13, 1), (9, 7, 1), (5, 4, 1), (3, 3, 1)],
    (65, 64, 1): [(65, 64, 1), (33, 33, 1), (17, 17, 1), (9, 9, 1), (5, 5, 1), (3, 3, 1)],
    (4, 4, 1): [(4, 4, 1), (3, 3, 1)],
    (16, 16, 16): [(16, 16, 16), (9, 9, 9), (5, 5, 5), (3, 3, 3)],
    (6, 4, 3): [(6, 4, 3), (4, 3, 3), (3, 3, 3)],
    (4, 5, 6): [(4, 5, 6), (3, 3, 4), (3, 3, 3)],
}


@functools.lru_cache(maxsize=None)
def _operator(grid):
    return S.AssembleOperator_Laplace3D(*grid) if grid[2] > 1 else S.AssembleOperator_Laplace(grid[0], grid[1])


def _build(grid, **kw):
    return S.AmgHierarchy(_operator(grid)[0], **dict(dict(coarsening="grid", grid=grid, coarse_eq_limit=10, sides="any"), **kw))


def _bytes(h):
    """every matrix of every level, and lambda_max"""
    info = h.info()
    L = info["levels"]
    out = [np.array(info["lambda_max"]).tobytes(), repr(info["dims"]).encode()]
    for l in range(L):
        for w in [S.AMG_OP] + ([S.AMG_PROLONG] if l + 1 < L else [S.AMG_COARSE_INV]):
            out += [a.tobytes() for a in h.matrix(l, w)[:3]]
    return out


@pytest.mark.parametrize("grid,bs", GRIDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"bs{v}")
def test_grids_and_prolongators_of_every_level(grid, bs):
    h = _build(grid)
    info = h.info()
    dims = level_dims(grid, bs)
    assert info["sides"] == S.AMG_SIDES_ANY and info["coarsening"] == S.AMG_COARSEN_GRID and info["block_size"] == bs
    assert info["dims"] == dims and info["levels"] == len(dims) >= 2
    if grid in EXPECT_DIMS:
        assert dims == EXPECT_DIMS[grid]
    assert info["rows"] == [bs * int(np.prod(d)) for d in dims]
    for l in range(info["levels"] - 1):
        rp, ci, v, shape = h.matrix(l, S.AMG_PROLONG)
        ref = prolong_ref(dims[l], bs)
        assert shape == ref.shape == (info["rows"][l], info["rows"][l + 1])
        assert rp.tobytes() == ref.indptr.astype(np.int32).tobytes(), (grid, l)
        assert ci.tobytes() == ref.indices.astype(np.int32).tobytes(), (grid, l)
        assert v.tobytes() == ref.data.astype(np.float64).tobytes(), (grid, l)
        # the Galerkin product with R = P^T, exactly symmetric
        P = sp.csr_matrix((v, ci, rp), shape=shape)
        Al, Ac = (sp.csr_matrix((m[2], m[1], m[0]), shape=m[3]) for m in (h.matrix(l, S.AMG_OP), h.matrix(l + 1, S.AMG_OP)))
        G = (P.T @ Al @ P).toarray()
        assert np.linalg.norm(Ac.toarray() - 0.5 * (G + G.T)) <= 1e-13 * np.linalg.norm(G)
        assert (Ac != Ac.T).nnz == 0
    h.close()


# ---- 3. `any` where every side is odd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(33, 17, 1), (17, 17, 17)])
def test_any_on_odd_sides_is_odd_byte_for_byte(grid):
    a, o = _build(grid), _build(grid, sides="odd")
    assert a.info()["sides"] == S.AMG_SIDES_ANY and o.info()["sides"] == S.AMG_SIDES_ODD
    assert a.info()["dims"] == level_dims(grid, 3 if grid[2] > 1 else 2, "odd")
    assert _bytes(a) == _bytes(o)
    a.close(), o.close()


# ---- 4. the option's values ------------------------------------------------------------------------------------------------------
def test_option_values():
    d = S.solver.amg_opts_dict(S.amg_opts())
    assert d["sides"] == S.AMG_SIDES_ODD == 0 and S.AMG_SIDES_ANY == 1
    assert S.solver.amg_opts_dict(S.amg_opts(sides="any"))["sides"] == S.AMG_SIDES_ANY
    A = _operator((6, 6, 1))[0]
    for bad in (2, -1):
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A, coarsening="grid", grid=(6, 6), sides=bad)
        assert e.value.code == SPK_ERR_ARG and "sides" in str(e.value)
    # under aggregation the field is not read
    A17 = _operator((17, 17, 1))[0]
    h0, h1, h2 = S.AmgHierarchy(A17), S.AmgHierarchy(A17, sides="any"), S.AmgHierarchy(A17, sides=2)
    assert h1.info()["sides"] == 0 and h1.info()["coarsening"] == S.AMG_COARSEN_AGGREGATION
    assert _bytes(h0) == _bytes(h1) == _bytes(h2)
    for h in (h0, h1, h2):
        h.close()


# ---- 5. the facade (no GPU: SetFromOptions runs before any context exists) and the refusal's text ------------------------
@pytest.mark.parametrize("prefix", ["", "-fieldsplit_0_"])
def test_facade_reads_back_the_side_rule(prefix):
    k = S.KSP()
    pc = ["-pc_type", "mg"] if not prefix else ["-pc_type", "fieldsplit", "-fieldsplit_0_ksp_type", "preonly", "-fieldsplit_0_pc_type", "mg"]
    key = prefix + "spk_mg_sides" if prefix else "-spk_mg_sides"
    k.setFromOptions(["-ksp_type", "fgmres"] + pc)
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["sides"] == S.AMG_SIDES_ODD
    k.setFromOptions([key, "any"])
    got, sel = k.getAMGOptions(fieldsplit0=bool(prefix))
    other, osel = k.getAMGOptions(fieldsplit0=not prefix)
    assert sel and not osel and got["sides"] == S.AMG_SIDES_ANY and other["sides"] == S.AMG_SIDES_ODD
    k.setFromOptions([key, "odd"])
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["sides"] == S.AMG_SIDES_ODD
    for opts, code in (([key, "even"], SPK_ERR_UNSUPPORTED), ([key, "1"], SPK_ERR_UNSUPPORTED), ([key], SPK_ERR_ARG)):
        with pytest.raises(SpkError) as e:
            k.setFromOptions(opts)
        assert e.value.code == code, opts
    k.destroy()
    k = S.KSP()   # without mg selected: read and not used
    k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "gamg", "-spk_mg_sides", "any"])
    got, sel = k.getAMGOptions()
    assert sel and got["coarsening"] == S.AMG_COARSEN_AGGREGATION and got["sides"] == S.AMG_SIDES_ANY
    k.destroy()


def test_the_odd_refusal_names_the_option():
    A = _operator((64, 64, 1))[0]
    for kw in ({}, dict(sides="odd")):
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A, coarsening="grid", grid=(64, 64), **kw)
        assert e.value.code == SPK_ERR_UNSUPPORTED
        assert "side of 64 nodes" in str(e.value) and "-spk_mg_sides any" in str(e.value)
    h = S.AmgHierarchy(A, coarsening="grid", grid=(64, 64), sides="any")   # default limit of 50 equations
    assert h.info()["dims"] == [(64, 64, 1), (33, 33, 1), (17, 17, 1), (9, 9, 1), (5, 5, 1)]
    h.close()


# ---- 6. the refresh ------------------------------------------------------------------------------------------------------------
def test_refresh_keeps_p_bit_for_bit():
    mx, my = 64, 48
    A0 = _operator((mx, my, 1))[0]
    kappa = 1.0 + np.random.default_rng(7).random((mx - 1) * (my - 1))
    A1 = S.AssembleOperator_Laplace(mx, my, kappa=kappa)[0]
    assert np.array_equal(A0.colidx, A1.colidx) and not np.array_equal(A0.val, A1.val)
    h = _build((mx, my, 1))
    i0 = h.info()
    P0 = [h.matrix(l, S.AMG_PROLONG) for l in range(i0["levels"] - 1)]
    h.refresh(A1.val)
    i1 = h.info()
    assert i1["dims"] == i0["dims"] and i1["sides"] == S.AMG_SIDES_ANY and i1["lambda_max"] != i0["lambda_max"]
    for l, p0 in enumerate(P0):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(h.matrix(l, S.AMG_PROLONG)[:3], p0[:3])), f"P_{l}"
    fresh = S.AmgHierarchy(A1, coarsening="grid", grid=(mx, my), coarse_eq_limit=10, sides="any")
    assert _bytes(h) == _bytes(fresh)   # the host route refreshes by the products that build
    h.close(), fresh.close()


# ---- 7. the numpy V-cycle as a CG preconditioner ------------------------------------------------------------------------------
def vcycle_ref(A, P, Ci, lam, b, smooth_its=2, esteig=(0, 0.1, 0, 1.1)):
    """One V-cycle as the library runs it (test_amg_cpu.vcycle_ref, Chebyshev only): nu steps
    y+ = y + alpha D^-1 (b - A y) + beta (y - y-) from zero, the residual restricted by P^T, recursion, y += P e, nu steps
    from y; the coarsest level y = C b.  Chebyshev coefficients of Saad Alg. 12.1 over [0.1, 1.1] lambda_max."""
    L = len(A)
    dinv = [1.0 / np.where(a.diagonal() == 0.0, 1.0, a.diagonal()) for a in A]
    coef = []
    for l in range(L - 1):
        lo, hi = esteig[1] * lam[l], esteig[3] * lam[l]
        th, de = 0.5 * (hi + lo), 0.5 * (hi - lo)
        sg = th / de
        rho = 1.0 / sg
        al, be = [1.0 / th], [0.0]
        for _ in range(1, smooth_its):
            rn = 1.0 / (2.0 * sg - rho)
            al.append(2.0 * rn / de)
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
                    yn = yn + be * (y - (prev if prev is not None else 0.0))
            prev, y = y, yn
        return y

    def rec(l, bb):
        if l == L - 1:
            return Ci @ bb
        y = smooth(l, bb, None)
        e = rec(l + 1, P[l].T @ (bb - A[l] @ y))
        return smooth(l, bb, y + P[l] @ e)

    return rec(0, np.asarray(b, np.float64))


def hierarchy_mats(get, info):
    to_sp = lambda m: sp.csr_matrix((m[2], m[1], m[0]), shape=m[3])
    L = info["levels"]
    return ([to_sp(get(l, S.AMG_OP)) for l in range(L)], [to_sp(get(l, S.AMG_PROLONG)) for l in range(L - 1)],
            to_sp(get(L - 1, S.AMG_COARSE_INV)).toarray())


def _pcg_its(n, sides, rtol=1e-8):
    A, f = S.AssembleOperator_Laplace(n, n)
    Asp = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))
    h = S.AmgHierarchy(A, coarsening="grid", grid=(n, n), sides=sides)
    info = h.info()
    mats = hierarchy_mats(h.matrix, info)
    h.close()
    M = spl.LinearOperator(Asp.shape, matvec=lambda r: vcycle_ref(*mats, info["lambda_max"], r))
    cnt = [0]
    x, rc = spl.cg(Asp, f, M=M, rtol=rtol, maxiter=200, callback=lambda xk: cnt.__setitem__(0, cnt[0] + 1))
    assert rc == 0 and np.linalg.norm(f - Asp @ x) <= 10 * rtol * np.linalg.norm(f)
    return cnt[0], info


@pytest.mark.parametrize("m", [64, 128])
def test_vcycle_iterations_on_an_even_grid_match_the_odd_grid_one_larger(m):
    """K = A of the 2-D generator, V-cycle-preconditioned CG to rtol 1e-8: iterations(any, m) <= iterations(odd, m + 1) + 1
    (the +1 is the project's parity bar for iteration counts).  Measured: 64^2 any 8 against 65^2 odd 8; 128^2 any 8
    against 129^2 odd 8."""
    even, ie = _pcg_its(m, "any")
    odd, io = _pcg_its(m + 1, "odd")
    print(f"{m}^2 any: {even} iterations, {ie['levels']} levels, complexity {ie['operator_complexity']:.3f}; "
          f"{m + 1}^2 odd: {odd} iterations, {io['levels']} levels, complexity {io['operator_complexity']:.3f}")
    assert ie["levels"] == io["levels"] and ie["dims"][1:] == io["dims"][1:]
    assert even <= odd + 1
