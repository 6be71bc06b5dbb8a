"""The exact Schur complement of a few constraint rows on the device (schur_pre="full",
-pc_fieldsplit_schur_precondition full): S = B A^ ^-1 B^T dense and Cholesky-factored, W = A^ ^-1 B^T kept, A^ ^-1 the
V-cycle (gamg) or diag(A)^-1.  The numpy side is vcycle_ref over the context's exported hierarchy, dense B and np.linalg.

Bars.  One V-cycle against numpy: the project's 1e-12 (test_gpu_amg); a vector kernel against numpy: 1e-13
(test_gpu_general_b.KERNEL_TOL).  S itself is held to those.  One PCApply solves with S, which multiplies the rounding
of its right-hand side by at most cond(S): its bar is that figure times cond(S) as numpy computes it from its own S."""
import functools
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from test_amg_cpu import general_spd, hierarchy_mats, vcycle_ref
from test_minres_cpu import minres_ref

pytestmark = pytest.mark.gpu
SPK_ERR_STATE, SPK_ERR_UNSUPPORTED = -3, -6
MARKER = -7777777.0
VCYCLE_TOL, KERNEL_TOL = 1e-12, 1e-13
FACTS = ("DIAG", "LOWER", "UPPER", "FULL")
# the shared shapes: an odd non-square grid, 33^2, an odd general (0,0) block (n_local = 1001) under five random rows, the
# 9^3 cube with its six rows (n_local = 2187, odd), and blocks of 1, 3 and 8 rows cut from the 24 x 17 grid's four
SHAPES = ("g24x17", "g33", "gen1001_b5", "cube9", "g24x17_m1", "g24x17_m3", "g24x17_m8")
_CTX, _REF = {}, {}


def _csr(M):
    return sp.csr_matrix((M.val, M.colidx, M.rowptr), shape=(M.nrows, M.ncols))


def _from_dense(S, Bd):
    rp = np.concatenate([[0], np.cumsum((Bd != 0).sum(1))]).astype(np.int32)
    return S.CSR(rp, np.concatenate([np.nonzero(r)[0] for r in Bd]).astype(np.int32), Bd[Bd != 0], Bd.shape[1])


def _split_rows(Bd, pieces):
    """every row cut into `pieces` rows over consecutive column ranges (disjoint supports: independent when none is empty)"""
    n = Bd.shape[1]
    cuts = [n * k // pieces for k in range(pieces + 1)]
    out = np.zeros((Bd.shape[0] * pieces, n))
    for r in range(Bd.shape[0]):
        for k in range(pieces):
            out[r * pieces + k, cuts[k]:cuts[k + 1]] = Bd[r, cuts[k]:cuts[k + 1]]
    assert np.all((out != 0).sum(1) > 0)
    return out


@functools.lru_cache(maxsize=None)
def _shape(name):
    """dict(A, B, Asp, Bd (dense), K (scipy CSC of the whole system), rhs, n, m)"""
    import saddle_point_petsc_amd as S
    if name.startswith("g") and name[1].isdigit():
        grid = {"g24x17": (24, 17), "g33": (33, 33), "g64": (64, 64), "g128": (128, 128)}[name.split("_")[0]]
        A, f = S.AssembleOperator_Laplace(*grid)
        B, g = S.AssembleOperator_Constraints(*grid)
        Asp = _csr(A)
        if "_m" in name:
            m = int(name.split("_m")[1])
            Bd = _csr(B).toarray()
            Bd = _split_rows(Bd, (m + 3) // 4)[:m] if m > 4 else Bd[:m]
            B, g = _from_dense(S, Bd), np.linspace(0.5, 1.5, m)
    elif name == "cube9":
        A, f = S.AssembleOperator_Laplace3D(9, 9, 9)[:2]
        B, g = S.AssembleOperator_Constraints3D(9, 9, 9)
        Asp = _csr(A)
    else:
        assert name == "gen1001_b5"
        A, Asp = general_spd(1001, 1001)
        rng = np.random.default_rng(1006)
        f, g = rng.standard_normal(1001), rng.standard_normal(5)
        B = _from_dense(S, np.where(rng.random((5, 1001)) < 0.4, rng.standard_normal((5, 1001)), 0.0))
    Bsp = _csr(B)
    K = sp.bmat([[Asp, Bsp.T], [Bsp, None]], format="csc")
    return dict(A=A, B=B, Asp=Asp.tocsr(), Bd=Bsp.toarray(), K=K, rhs=np.concatenate([f, g]), n=A.nrows, m=B.nrows)


def _ctx(spk, name, amg, fact="FULL", pre="full"):
    """one context per shape and A^ for the whole module, set up again for the factorisation asked for"""
    key = (name, bool(amg))
    if key not in _CTX:
        sh = _shape(name)
        c = spk.Context(0)
        c.set_block(spk.BLOCK_A00, sh["A"])
        c.set_block(spk.BLOCK_A10, sh["B"])
        _CTX[key] = c
    c = _CTX[key]
    c.pc_setup(spk.PC_SCHUR, getattr(spk, "SCHUR_" + fact), amg=amg if amg else None, schur_pre=pre)
    return c


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()
    _REF.clear()


def _ref(spk, name, amg):
    """numpy's A^ ^-1 (a callable), W = A^ ^-1 B^T, S = B W symmetrised and cond(S); the hierarchy is the context's own,
    exported once (every set-up of one context builds the same one)"""
    key = (name, bool(amg))
    if key not in _REF:
        sh = _shape(name)
        if amg:
            c = _ctx(spk, name, amg)
            info = c.amg_info()
            mats = hierarchy_mats(c.amg_level, info)
            ainv = lambda v: vcycle_ref(*mats, info["lambda_max"], v)   # noqa: E731
        else:
            d = sh["Asp"].diagonal()
            dinv = 1.0 / np.where(d == 0.0, 1.0, d)
            ainv = lambda v: dinv * v   # noqa: E731
        W = np.stack([ainv(sh["Bd"][r]) for r in range(sh["m"])], axis=1)
        G = sh["Bd"] @ W
        S = 0.5 * (G + G.T)
        _REF[key] = dict(ainv=ainv, W=W, S=S, G=G, cond=np.linalg.cond(S))
    return _REF[key]


def _apply_ref(sh, R, fact, x):
    """the block algebra of include/spk.h, t = B A^ ^-1 x0 formed through B"""
    n = sh["n"]
    x0, x1 = x[:n], x[n:]
    a = R["ainv"](x0)
    t = sh["Bd"] @ a
    if fact == "DIAG":
        return np.concatenate([a, np.linalg.solve(R["S"], x1)])
    if fact == "LOWER":
        return np.concatenate([a, np.linalg.solve(R["S"], t - x1)])
    y1 = -np.linalg.solve(R["S"], x1) if fact == "UPPER" else np.linalg.solve(R["S"], t - x1)
    return np.concatenate([a - R["W"] @ y1, y1])


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


# ---- the kernels alone: every m, the ends of the vector, the grid-stride path ------------------------------------------
def _kernel_case(spk, c, nl, m, fact, jac, seed):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((m, nl))
    Lf = np.tril(rng.standard_normal((m, m)), -1) * 0.3 + np.diag(1.0 + rng.random(m))
    S = Lf @ Lf.T
    x = rng.standard_normal(nl + m)
    src = None if jac else rng.standard_normal(nl)
    dinv = 1.0 + rng.random(nl) if jac else None
    y = c.debug_schur_w(W, Lf, x, fact=getattr(spk, "SCHUR_" + fact), src=src, dinv=dinv, pad=np.nan)
    assert np.all(y[nl + m:] == MARKER)                       # nothing behind the vector
    x0, x1 = x[:nl], x[nl:]
    t = W @ x0
    y1 = {"DIAG": lambda: np.linalg.solve(S, x1), "UPPER": lambda: -np.linalg.solve(S, x1)}.get(
        fact, lambda: np.linalg.solve(S, t - x1))()
    bar = KERNEL_TOL * np.linalg.cond(S)
    # t is a sum of nl products of O(1) terms: its rounding is relative to sqrt(nl), not to a t that may cancel
    scale = np.linalg.norm(np.linalg.solve(S, np.full(m, np.sqrt(nl)) + np.abs(x1)))
    assert np.linalg.norm(y[nl:nl + m] - y1) <= bar * scale, (nl, m, fact, np.linalg.norm(y[nl:nl + m] - y1) / scale)
    if fact in ("UPPER", "FULL"):
        s = dinv * x0 if jac else src
        ref = s - y[nl:nl + m] @ W                            # the update with the device's own y1
        assert np.linalg.norm(y[:nl] - ref) <= KERNEL_TOL * np.linalg.norm(np.abs(s) + np.abs(y[nl:nl + m]) @ np.abs(W))
    else:
        assert np.all(y[:nl] == MARKER)


@pytest.mark.parametrize("m", range(1, 9))
def test_kernels_every_row_count_and_vector_end(spk, m):
    """n_local = 1, 2, 3 (less than a pair, a pair, a pair and a half), around the wave (63..65), around the 1024-entry tile
    (1023..1026) and several workgroups with an odd end; every factorisation, both forms of the source."""
    with spk.Context(0) as c:
        for i, nl in enumerate((1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 1026, 5001)):
            for j, fact in enumerate(FACTS):
                _kernel_case(spk, c, nl, m, fact, jac=(i + j) % 2 == 0, seed=100 * m + 10 * i + j)


@pytest.mark.parametrize("m,fact,jac", [(4, "FULL", False), (7, "FULL", True), (1, "LOWER", False)])
def test_kernels_beyond_one_tile_per_workgroup(spk, m, fact, jac):
    """more than 512 tiles of 1024 entries: the workgroups stride over the vector (the 1024^2 grid has 2048 tiles)"""
    with spk.Context(0) as c:
        _kernel_case(spk, c, 512 * 1024 + 2 * 1024 + 77, m, fact, jac, seed=m)


def test_kernels_take_the_gate(spk):
    rng = np.random.default_rng(5)
    W, Lf, x = rng.standard_normal((3, 700)), np.eye(3), rng.standard_normal(703)
    with spk.Context(0) as c:
        for fact in FACTS:
            y = c.debug_schur_w(W, Lf, x, fact=getattr(spk, "SCHUR_" + fact), done=1)
            assert np.all(y == MARKER), fact
            y = c.debug_schur_w(W, Lf, x, fact=getattr(spk, "SCHUR_" + fact), done=0)
            assert not np.any(y[700:703] == MARKER), fact


# ---- S ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amg", [False, True], ids=["D", "gamg"])
@pytest.mark.parametrize("name", SHAPES + ("g64",))
def test_schur_matrix_matches_numpy(spk, name, amg):
    sh = _shape(name)
    c = _ctx(spk, name, amg)
    S = c.schur_matrix()
    R = _ref(spk, name, amg)
    assert S.shape == (sh["m"], sh["m"]) and np.array_equal(S, S.T)
    err = _rel(S, R["S"])
    print(f"schur_matrix {name} {'gamg' if amg else 'D'}: rel err {err:.2e}, cond(S) {R['cond']:.1f}, "
          f"asymmetry of numpy's B W {np.abs(R['G'] - R['G'].T).max() / np.abs(R['G']).max():.1e}")
    assert err <= (VCYCLE_TOL if amg else KERNEL_TOL)
    assert np.array_equal(c.schur_diag(), _ctx(spk, name, amg, pre="selfp").schur_diag())   # spk_get_schur_diag keeps its meaning
    if not amg:
        assert _rel(np.diag(S), c.schur_diag()) <= KERNEL_TOL                                # with D, S^ is diag(S)


# ---- one PCApply --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amg", [False, True], ids=["D", "gamg"])
@pytest.mark.parametrize("name", SHAPES)
def test_pc_apply_matches_block_algebra(spk, name, amg):
    sh = _shape(name)
    R = _ref(spk, name, amg)
    bar = (VCYCLE_TOL if amg else KERNEL_TOL) * R["cond"]
    x = np.random.default_rng(sh["n"]).standard_normal(sh["n"] + sh["m"])
    for fact in FACTS:
        c = _ctx(spk, name, amg, fact)
        y = c.pc_apply(x)
        assert np.array_equal(y, c.pc_apply(x))
        err = _rel(y, _apply_ref(sh, R, fact, x))
        print(f"pc_apply {name} {'gamg' if amg else 'D'} {fact}: rel err {err:.2e} (bar {bar:.2e})")
        assert err <= bar, (fact, err, bar)


@pytest.mark.parametrize("amg", [False, True], ids=["D", "gamg"])
@pytest.mark.parametrize("name", SHAPES)
def test_full_is_exact_on_the_constraint_rows(spk, name, amg):
    """FULL with the exact S inverts [A^ B^T; B 0]: B y0 = x1 for any x (B y0 = t - S y1).  Today's S^ misses it by O(1)."""
    sh = _shape(name)
    R = _ref(spk, name, amg)
    n, Bd = sh["n"], sh["Bd"]
    bar = (VCYCLE_TOL if amg else KERNEL_TOL) * R["cond"]
    x = np.random.default_rng(sh["n"] + 1).standard_normal(sh["n"] + sh["m"])
    y = _ctx(spk, name, amg, "FULL").pc_apply(x)
    scale = np.linalg.norm(np.abs(Bd) @ np.abs(y[:n]) + np.abs(x[n:]))
    miss = np.linalg.norm(Bd @ y[:n] - x[n:])
    ys = _ctx(spk, name, amg, "FULL", pre="selfp").pc_apply(x)
    miss_selfp = np.linalg.norm(Bd @ ys[:n] - x[n:])
    print(f"B y0 - x1, {name} {'gamg' if amg else 'D'}: exact S {miss / scale:.2e} of the scale, selfp "
          f"{miss_selfp / np.linalg.norm(x[n:]):.2e} of ||x1||")
    assert miss <= bar * scale
    # S^ = diag(B D B^T) is the exact S only where A^ = D and the rows' supports are disjoint (the grids' own blocks): there
    # selfp is exact already; everywhere else it misses by O(1)
    offdiag = np.linalg.norm(R["S"] - np.diag(np.diag(R["S"]))) / np.linalg.norm(R["S"])
    if amg or offdiag > 1e-2:
        assert miss_selfp >= 0.05 * np.linalg.norm(x[n:]), (miss_selfp, offdiag)
    else:
        assert offdiag <= 1e-13 and miss_selfp <= bar * scale, (miss_selfp, offdiag)


# ---- solves --------------------------------------------------------------------------------------------------------------
def fgmres_ref(K, M, b, rtol, restart=30, max_it=10000):
    """textbook right-preconditioned FGMRES(restart), the test of KSPConvergedDefault on the recurrence's residual"""
    x = np.zeros_like(b)
    bn = np.linalg.norm(b)
    its = 0
    while its < max_it:
        r = b - K @ x
        beta = np.linalg.norm(r)
        if beta <= rtol * bn:
            break
        V, Z = [r / beta], []
        H = np.zeros((restart + 1, restart))
        for j in range(restart):
            Z.append(M(V[j]))
            w = K @ Z[j]
            for i in range(j + 1):
                H[i, j] = V[i] @ w
            for i in range(j + 1):
                w = w - H[i, j] * V[i]
            H[j + 1, j] = np.linalg.norm(w)
            V.append(w / H[j + 1, j])
            its += 1
            e1 = np.zeros(j + 2)
            e1[0] = beta
            yk, res = np.linalg.lstsq(H[:j + 2, :j + 1], e1, rcond=None)[:2]
            rn = np.linalg.norm(H[:j + 2, :j + 1] @ yk - e1)
            if rn <= rtol * bn or its >= max_it:
                break
        x = x + np.stack(Z, axis=1) @ yk
        if rn <= rtol * bn:
            break
    return x, its


@pytest.mark.parametrize("setup", ["host", "device"])
@pytest.mark.parametrize("name", ["g64", "g128"])
def test_full_gamg_solves(spk, name, setup):
    sh = _shape(name)
    K, rhs, n = sh["K"], sh["rhs"], sh["n"]
    amg = dict(setup=setup)
    c = _ctx(spk, name, amg, "FULL")
    assert c.amg_info()["setup"] == (spk.AMG_SETUP_DEVICE if setup == "device" else spk.AMG_SETUP_HOST)
    x, info = c.fgmres(rhs, rtol=1e-8, max_it=200)
    assert c.iteration_form()[0] == -1
    x10, i10 = c.fgmres(rhs, rtol=1e-10, max_it=200)
    # numpy's FGMRES with the same preconditioner: this context's hierarchy, S and W from it
    ai = c.amg_info()
    mats = hierarchy_mats(c.amg_level, ai)
    ainv = lambda v: vcycle_ref(*mats, ai["lambda_max"], v)   # noqa: E731
    W = np.stack([ainv(sh["Bd"][r]) for r in range(sh["m"])], axis=1)
    G = sh["Bd"] @ W
    R = dict(ainv=ainv, W=W, S=0.5 * (G + G.T))
    _, ref_its = fgmres_ref(K.tocsr(), lambda v: _apply_ref(sh, R, "FULL", v), rhs, 1e-8)
    _, selfp = _ctx(spk, name, amg, "FULL", pre="selfp").fgmres(rhs, rtol=1e-8, max_it=200)
    print(f"FULL + gamg ({setup}) at {name}: {info['its']} iterations, numpy {ref_its}, selfp {selfp['its']}")
    assert info["reason"] == 2 and selfp["reason"] == 2 and i10["reason"] == 2
    assert abs(info["its"] - ref_its) <= 1, (info["its"], ref_its)
    assert info["its"] < selfp["its"], (info["its"], selfp["its"])
    assert np.linalg.norm(rhs - K @ x) <= 1.0001e-8 * np.linalg.norm(rhs)
    assert _rel(x10, spl.spsolve(K, rhs)) <= 1e-8
    assert n == sh["A"].nrows


def test_identical_bits_selfp_afterwards_and_device_vectors(spk):
    sh = _shape("g64")
    rhs = sh["rhs"]

    def fresh(pre):
        c = spk.Context(0)
        c.set_block(spk.BLOCK_A00, sh["A"])
        c.set_block(spk.BLOCK_A10, sh["B"])
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL, amg=True, schur_pre=pre)
        return c

    with fresh("full") as c:
        x1, i1 = c.fgmres(rhs, rtol=1e-8)
        x2, i2 = c.fgmres(rhs, rtol=1e-8)
        assert i1["reason"] == 2
        assert np.array_equal(x1, x2) and np.array_equal(i1["history"], i2["history"])
        bd, xd = c.vec_create(rhs), c.vec_create(n=len(rhs))
        idev = c.fgmres_device(bd, xd, rtol=1e-8)
        xv = c.vec_get(xd, len(rhs))
        c.vec_destroy(bd)
        c.vec_destroy(xd)
        assert np.array_equal(xv, x1) and np.array_equal(idev["history"], i1["history"])
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL, amg=True)          # schur_pre="selfp" again
        with pytest.raises(spk.SpkError) as e:
            c.schur_matrix()
        assert e.value.code == SPK_ERR_STATE
        xs, isf = c.fgmres(rhs, rtol=1e-8, max_it=300)
    with fresh("selfp") as c:
        xf, ifr = c.fgmres(rhs, rtol=1e-8, max_it=300)
    assert np.array_equal(xs, xf) and np.array_equal(isf["history"], ifr["history"])
    # ... and without the V-cycle: the fused forms come back with their bits
    with fresh("selfp") as c:
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL, schur_pre="full")
        xe, ie = c.fgmres(rhs, rtol=1e-8, max_it=3000)
        assert c.iteration_form()[0] == -1 and c.bd_planes() == 0
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
        xs, isf = c.fgmres(rhs, rtol=1e-8, max_it=3000)
        form = c.iteration_form()
        planes = c.bd_planes()
    with spk.Context(0) as c:
        c.set_block(spk.BLOCK_A00, sh["A"])
        c.set_block(spk.BLOCK_A10, sh["B"])
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
        xf, ifr = c.fgmres(rhs, rtol=1e-8, max_it=3000)
        assert c.iteration_form() == form and c.bd_planes() == planes and form[0] != -1
    assert np.array_equal(xs, xf) and np.array_equal(isf["history"], ifr["history"])
    assert ie["reason"] == 2


def test_minres_diag_with_the_exact_complement(spk):
    """DIAG, A^ = D and the dense S: symmetric positive definite, so MINRES takes it -- on its step-by-step route, chosen
    by itself.  Against minres_ref with the same preconditioner in numpy; the saddle bar, 1e-8."""
    sh = _shape("g33")
    K, rhs = sh["K"].tocsr(), sh["rhs"]
    R = _ref(spk, "g33", False)
    M = lambda v: _apply_ref(sh, R, "DIAG", v)   # noqa: E731
    c = _ctx(spk, "g33", False, "DIAG")
    _, i20 = c.minres(rhs, rtol=0.0, abstol=0.0, max_it=20)
    x, info = c.minres(rhs, rtol=1e-8)
    _, u = c.minres(rhs, rtol=1e-8, fused=0)
    _, r20 = minres_ref(lambda v: K @ v, M, rhs, rtol=0.0, abstol=0.0, max_it=20)
    _, ref = minres_ref(lambda v: K @ v, M, rhs, rtol=1e-8)
    assert i20["its"] == 20 and i20["reason"] == -3
    err = np.max(np.abs(i20["history"] - r20["history"]) / np.abs(r20["history"]))
    print(f"minres + exact S at 33^2: history err {err:.2e}, {info['its']} iterations, numpy {ref['its']}")
    assert err <= 1e-8
    assert info["reason"] == 2 and ref["reason"] == 2
    assert abs(info["its"] - ref["its"]) <= max(2, ref["its"] // 100), (info["its"], ref["its"])
    assert np.linalg.norm(rhs - K @ x) <= 1.0001e-8 * np.linalg.norm(rhs)
    assert np.array_equal(u["history"], info["history"])      # opts.fused = 0 is the route it took by itself
    for fact in ("LOWER", "UPPER", "FULL"):
        with pytest.raises(spk.SpkError) as e:
            _ctx(spk, "g33", False, fact).minres(rhs, rtol=1e-8)
        assert e.value.code == SPK_ERR_UNSUPPORTED
    with pytest.raises(spk.SpkError) as e:
        _ctx(spk, "g33", True, "DIAG").minres(rhs, rtol=1e-8)  # MINRES + gamg stays refused
    assert e.value.code == SPK_ERR_UNSUPPORTED


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _usable(spk, c, rhs, K):
    c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
    x, info = c.fgmres(rhs, rtol=1e-8, max_it=5000)
    assert info["reason"] == 2
    assert np.linalg.norm(rhs - K @ x) <= 1.0001e-8 * np.linalg.norm(rhs)


def _refused(spk, c, *words, **kw):
    with pytest.raises(spk.SpkError) as e:
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL, schur_pre="full", **kw)
    assert e.value.code == SPK_ERR_UNSUPPORTED, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def _block_ctx(spk, A, B):
    c = spk.Context(0)
    c.set_block(spk.BLOCK_A00, A)
    c.set_block(spk.BLOCK_A10, B)
    return c


def test_refusals_keep_the_context_usable(spk):
    sh = _shape("g24x17")
    Asp, n = sh["Asp"], sh["n"]
    f = sh["rhs"][:n]

    def system(Bd):
        Bs = sp.csr_matrix(Bd)
        return sp.bmat([[Asp, Bs.T], [Bs, None]], format="csr"), np.concatenate([f, np.linspace(0.5, 1.5, Bd.shape[0])])

    # nine rows
    B9 = _split_rows(sh["Bd"], 3)[:9]
    K9, rhs9 = system(B9)
    with _block_ctx(spk, sh["A"], _from_dense(spk, B9)) as c:
        _refused(spk, c, "8 constraint rows", "9")
        _refused(spk, c, "8 constraint rows", amg=True)
        _usable(spk, c, rhs9, K9)
    # inner sweeps
    with _block_ctx(spk, sh["A"], sh["B"]) as c:
        _refused(spk, c, "FP32", inner_sweeps=2)
        _usable(spk, c, sh["rhs"], sh["K"])
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL, schur_pre="full")      # ... and the mode itself afterwards
        assert c.schur_matrix().shape == (4, 4)
    # a repeated row: S is singular
    Bdup = np.vstack([sh["Bd"][:3], sh["Bd"][1:2]])
    for amg in (None, True):
        with _block_ctx(spk, sh["A"], _from_dense(spk, Bdup)) as c:
            c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL, amg=amg)
            _refused(spk, c, "positive definite", "rank-deficient", amg=amg)
            with pytest.raises(spk.SpkError) as e:
                c.schur_matrix()
            assert e.value.code == SPK_ERR_STATE
            c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL, amg=amg)             # selfp divides by S^ entry by entry: it sets up
            assert np.all(c.schur_diag() > 0)
    # a selfp set-up has no dense S
    with _block_ctx(spk, sh["A"], sh["B"]) as c:
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
        with pytest.raises(spk.SpkError) as e:
            c.schur_matrix()
        assert e.value.code == SPK_ERR_STATE
        c.pc_setup(spk.PC_JACOBI, schur_pre="full")                      # no effect unless the PC is the Schur split
        with pytest.raises(spk.SpkError) as e:
            c.schur_matrix()
        assert e.value.code == SPK_ERR_STATE


def test_general_block_refused_and_usable(spk):
    grid = (12, 10, 9)   # the general block of test_gpu_minres.test_general_constraint_block
    A, f = spk.AssembleOperator_Laplace3D(*grid)[:2]
    Bm, g = spk.AssembleOperator_Constraints3D(*grid)
    Bd = spk.AssembleOperator_Divergence3D(*grid)
    B = spk.CSR.vstack([Bm, Bd])
    x = np.random.default_rng(2).standard_normal(A.nrows + B.nrows)
    with _block_ctx(spk, A, B) as c:
        assert c.sizes()["m"] > 8
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
        y = c.pc_apply(x)
        _refused(spk, c, "8 constraint rows", "general")
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
        assert np.array_equal(c.pc_apply(x), y)


def test_two_rank_group_refused_and_usable(spk):
    P = 2
    sh = _shape("g33")
    grp = spk.LocalGroup(P)
    codes, infos, errs = [None] * P, [None] * P, []

    def work(r):
        try:
            b, e = spk.partition_slab(33, 33, r, P)
            As, _ = spk.AssembleOperator_Laplace(33, 33, b, e)
            Bs, _ = spk.AssembleOperator_Constraints(33, 33, b, e)
            c = spk.Context(0)
            c.comm_init_local(grp, r)
            c.set_block(spk.BLOCK_A00, As)
            c.set_block(spk.BLOCK_A10, Bs)
            try:
                c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL, schur_pre="full")
            except spk.SpkError as ex:
                codes[r] = (ex.code, str(ex))
            c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)                  # the context stays usable
            _, infos[r] = c.fgmres(np.concatenate([sh["rhs"][b:e], sh["rhs"][sh["n"]:]]), rtol=1e-8, max_it=5000)
            c.close()
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            raise

    th = [threading.Thread(target=work, args=(r,)) for r in range(P)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    grp.close()
    assert not errs, errs
    for code in codes:
        assert code is not None and code[0] == SPK_ERR_UNSUPPORTED and "one rank" in code[1]
    assert all(i["reason"] == 2 for i in infos) and infos[0]["its"] == infos[1]["its"]


# ---- the facade and the runner -------------------------------------------------------------------------------------------
def test_facade_and_runner(spk):
    sh = _shape("g64")
    opts = ("-ksp_type fgmres -ksp_rtol 1e-8 -pc_type fieldsplit -pc_fieldsplit_type schur -pc_fieldsplit_schur_fact_type full "
            "-fieldsplit_0_ksp_type preonly -fieldsplit_0_pc_type gamg -pc_fieldsplit_schur_precondition full")
    for extra in ("", " -fieldsplit_1_pc_type cholesky", " -fieldsplit_1_pc_type lu"):
        k = spk.KSP()
        k.setOperators(sh["A"], sh["B"])
        k.setFromOptions(opts + extra)
        x = k.solve(sh["rhs"])
        assert k.getConvergedReason() == 2 and k.getSchurPre() == ("full", "cholesky")
        its = k.getIterationNumber()
        k.destroy()
        c = _ctx(spk, "g64", True, "FULL")
        xc, info = c.fgmres(sh["rhs"], rtol=1e-8)
        assert np.array_equal(x, xc) and its == info["its"]
    k = spk.KSP()
    k.setOperators(sh["A"], sh["B"])
    k.setFromOptions(opts + " -fieldsplit_1_pc_type jacobi")
    with pytest.raises(spk.SpkError) as e:
        k.setUp()
    assert e.value.code == SPK_ERR_UNSUPPORTED and "-fieldsplit_1_pc_type" in str(e.value)
    k.destroy()

    exe = os.path.join(os.path.dirname(spk.LIB_PATH), "saddle_point_run")
    wd = tempfile.mkdtemp()
    args = ["-da_grid_x", "64", "-da_grid_y", "64", "-ksp_rtol", "1e-8", "-ksp_converged_reason", "-no_vtk", "-ksp_view"] + opts.split()[4:]
    out = subprocess.run([exe, "-ksp_type", "fgmres"] + args, capture_output=True, text=True, timeout=120, cwd=wd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout
    assert "schur_precondition full" in out.stdout and "m = 4" in out.stdout, out.stdout
    out = subprocess.run([exe, "-ksp_type", "fgmres"] + args[:-2], capture_output=True, text=True, timeout=120, cwd=wd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "schur_precondition selfp" in out.stdout and "m = 4" in out.stdout, out.stdout
