"""-spk_mg_galerkin stencil on the host route (no GPU): the coarse operators of a grid-coarsened hierarchy as a gather on
the node grid (include/spk.h, SPK_AMG_GALERKIN_STENCIL; csrc/spk_galerkin_core.hpp) -- the closed-form pattern, the values
level by level against scipy's P^T A_l P, bitwise symmetry, the children against the stored P, parity with the products
route, the refresh, the refusals, the defaults, the stand-alone host program under the sanitizers and the kernels'
resource remarks."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError
from test_mg_grid_cpu import five_point
from test_mg_sides_cpu import hierarchy_mats, level_dims, prolong_ref, vcycle_ref

SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6
U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# name -> (grid, bs, sides, operator)
SHAPES = {
    "5x5": ((5, 5, 1), 2, "odd", lambda: S.AssembleOperator_Laplace(5, 5)[0]),            # one interior coarse node
    "33x9": ((33, 9, 1), 2, "odd", lambda: S.AssembleOperator_Laplace(33, 9)[0]),         # semi-coarsening
    "12x9": ((12, 9, 1), 2, "odd", lambda: S.AssembleOperator_Laplace(12, 9)[0]),         # x never halves
    "12x10any": ((12, 10, 1), 2, "any", lambda: S.AssembleOperator_Laplace(12, 10)[0]),   # the single-child last node, even then odd
    "7x6any": ((7, 6, 1), 2, "any", lambda: S.AssembleOperator_Laplace(7, 6)[0]),
    "4x4any": ((4, 4, 1), 2, "any", lambda: S.AssembleOperator_Laplace(4, 4)[0]),
    "9x9x5": ((9, 9, 5), 3, "odd", lambda: S.AssembleOperator_Laplace3D(9, 9, 5)[0]),
    "6x4x3any": ((6, 4, 3), 3, "any", lambda: S.AssembleOperator_Laplace3D(6, 4, 3)[0]),
    "five17x9": ((17, 9, 1), 1, "odd", lambda: five_point(17, 9)),                        # no corner entries on level 0
}


@functools.lru_cache(maxsize=None)
def operator(name):
    return SHAPES[name][3]()


def amg_kw(name, **kw):
    grid, bs, sides, _ = SHAPES[name]
    return dict(dict(coarsening="grid", grid=grid, sides=sides, block_size=bs, coarse_eq_limit=10), **kw)


def build(name, A=None, **kw):
    return S.AmgHierarchy(operator(name) if A is None else A, **amg_kw(name, **kw))


def to_sp(m):
    return sp.csr_matrix((m[2], m[1], m[0]), shape=m[3])


def level_bytes(h, which=S.AMG_OP, first=0):
    info = h.info()
    last = info["levels"] - (1 if which == S.AMG_PROLONG else 0)
    return [tuple(a.tobytes() for a in h.matrix(l, which)[:3]) for l in range(first, last)]


def all_bytes(h):
    info = h.info()
    return (level_bytes(h), level_bytes(h, S.AMG_PROLONG), h.matrix(info["levels"] - 1, S.AMG_COARSE_INV)[2].tobytes(),
            np.array(info["lambda_max"]).tobytes())


@pytest.fixture(scope="module", params=list(SHAPES))
def built(request):
    h, g = build(request.param, galerkin="stencil"), build(request.param)
    yield request.param, h, g
    h.close(), g.close()


def stencil_pattern(d, bs):
    """the closed form in numpy: per node row the full bs x bs blocks of the clipped 3^d-node neighbourhood, ascending"""
    nx, ny, nz = d
    rp, ci = [0], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                cols = [((k2 * ny + j2) * nx + i2) * bs + b
                        for k2 in range(max(k - 1, 0), min(k + 1, nz - 1) + 1) for j2 in range(max(j - 1, 0), min(j + 1, ny - 1) + 1)
                        for i2 in range(max(i - 1, 0), min(i + 1, nx - 1) + 1) for b in range(bs)]
                for _ in range(bs):
                    ci += cols
                    rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32)


# ---- 1. the pattern ----------------------------------------------------------------------------------------------------
def test_pattern_is_the_closed_form(built):
    name, h, _ = built
    grid, bs, sides, _ = SHAPES[name]
    info = h.info()
    dims = level_dims(grid, bs, sides)
    assert info["galerkin"] == S.AMG_GALERKIN_STENCIL == 1 and info["dims"] == dims and info["levels"] == len(dims) >= 2
    nnz = [int(operator(name).rowptr[-1])]
    for l in range(1, info["levels"]):
        rp, ci, v, shape = h.matrix(l)
        erp, eci = stencil_pattern(dims[l], bs)
        assert shape == (bs * int(np.prod(dims[l])),) * 2
        assert rp.tobytes() == erp.tobytes() and ci.tobytes() == eci.tobytes(), (name, l)
        assert len(v) == len(eci) == bs * bs * int(np.prod([3 * n - 2 for n in dims[l]]))
        nnz.append(len(eci))
    assert info["nnz"] == nnz
    assert info["operator_complexity"] == pytest.approx(sum(nnz) / nnz[0], rel=1e-15)


# ---- 2, 3. the values level by level, and symmetry ---------------------------------------------------------------------
def test_values_against_scipy_level_by_level_and_bitwise_symmetry(built):
    """|A_{l+1} - (G + G^T) / 2| <= 2 9^d 2^-53 T entrywise, G = P^T A_l P from the route's own A_l and stored P, T = (|P|^T
    |A_l| |P| + its transpose) / 2: at most 9^d exact products per sum, 9^d - 1 roundings in ours, fewer in scipy's, one in each
    symmetrisation.  Largest ratios found: 0.028 of the bound in 2-D (12x10 any), 0.0083 in 3-D (9x9x5)."""
    name, h, _ = built
    grid = SHAPES[name][0]
    d = 3 if grid[2] > 1 else 2
    info = h.info()
    worst = 0.0
    for l in range(info["levels"] - 1):
        A, P, N = to_sp(h.matrix(l)), to_sp(h.matrix(l, S.AMG_PROLONG)), to_sp(h.matrix(l + 1))
        G = (P.T @ A @ P).tocsr()
        ref = (0.5 * (G + G.T)).toarray()
        T = (abs(P).T @ abs(A) @ abs(P)).toarray()
        bound = 2.0 * 9 ** d * U * 0.5 * (T + T.T)
        err = np.abs(N.toarray() - ref)
        assert np.all(err <= bound), (name, l, float((err - bound).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert np.all(N.toarray()[bound == 0] == 0.0)
        Nt = N.T.tocsr()
        Nt.sort_indices()
        assert Nt.indptr.tobytes() == N.indptr.tobytes() and Nt.indices.tobytes() == N.indices.tobytes()
        assert Nt.data.tobytes() == N.data.tobytes(), f"{name}: A_{l + 1} is not bitwise symmetric"
    print(f"{name}: largest |A_l+1 - ref| / bound = {worst:.4f}")


# ---- 4. the same rule as P ---------------------------------------------------------------------------------------------
def test_children_are_the_columns_of_the_stored_p(built):
    name, h, _ = built
    grid, bs, sides, _ = SHAPES[name]
    info = h.info()
    for l in range(info["levels"] - 1):
        P = to_sp(h.matrix(l, S.AMG_PROLONG)).tocsc()
        P.sort_indices()
        ref = prolong_ref(info["dims"][l], bs, sides)
        assert (abs(P - ref)).nnz == 0
        for C in range(int(np.prod(info["dims"][l + 1]))):
            nodes, w = S.amg_stencil_children(info["dims"][l], info["dims"][l + 1], C)
            for a in range(bs):
                col = C * bs + a
                rows, vals = P.indices[P.indptr[col]:P.indptr[col + 1]], P.data[P.indptr[col]:P.indptr[col + 1]]
                assert np.array_equal(rows, nodes * bs + a) and vals.tobytes() == w.tobytes(), (name, l, C)


def test_children_hook_refuses_what_is_no_coarsening():
    for args in (((5, 5, 1), (4, 3, 1), 0), ((5, 5, 1), (3, 3, 1), 9), ((5, 5, 1), (3, 3, 1), -1)):
        with pytest.raises(SpkError) as e:
            S.amg_stencil_children(*args)
        assert e.value.code == SPK_ERR_ARG


# ---- 5. against the products route -------------------------------------------------------------------------------------
def _its(h, Asp, f, ksp):
    info = h.info()
    mats = hierarchy_mats(h.matrix, info)
    M = spl.LinearOperator(Asp.shape, matvec=lambda r: vcycle_ref(*mats, info["lambda_max"], r))
    cnt = [0]
    if ksp == "cg":
        x, rc = spl.cg(Asp, f, M=M, rtol=1e-8, maxiter=200, callback=lambda xk: cnt.__setitem__(0, cnt[0] + 1))
    else:
        x, rc = spl.gmres(Asp, f, M=M, rtol=1e-8, restart=30, maxiter=200, callback=lambda rk: cnt.__setitem__(0, cnt[0] + 1),
                          callback_type="pr_norm")
    assert rc == 0
    return cnt[0]


def test_same_levels_and_iterations_as_the_products_route(built):
    name, h, g = built
    hi, gi = h.info(), g.info()
    assert gi["galerkin"] == S.AMG_GALERKIN_PRODUCTS == 0
    assert hi["levels"] == gi["levels"] and hi["dims"] == gi["dims"] and hi["rows"] == gi["rows"]
    dev = 0.0
    for l in range(1, hi["levels"]):
        a, b = to_sp(h.matrix(l)), to_sp(g.matrix(l))
        dev = max(dev, abs(a - b).max() / abs(b).max())
    Asp = to_sp(h.matrix(0))
    f = np.random.default_rng(11).standard_normal(Asp.shape[0])
    its = {k: (_its(h, Asp, f, k), _its(g, Asp, f, k)) for k in ("cg", "gmres")}
    print(f"{name}: stencil / products iterations {its}, nnz {hi['nnz']} / {gi['nnz']}, "
          f"largest entrywise deviation of an A_l {dev:.2e} of its largest entry (reported, not asserted)")
    for k, (a, b) in its.items():
        assert abs(a - b) <= 1, (name, k, a, b)


# ---- 6. the refresh ----------------------------------------------------------------------------------------------------
def _scaled(name):
    """the same pattern with other values: a kappa field through the generator, a positive diagonal scaling for five_point"""
    grid, bs, _, _ = SHAPES[name]
    rng = np.random.default_rng(7)
    if name.startswith("five"):
        A = operator(name)
        d = 1.0 + 0.01 * rng.random(A.nrows)   # (sum |D^-1| stays in its binade, 37.3 -> above 36.5: the refresh rescales nothing)
        M = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))
        M = (sp.diags(d) @ M @ sp.diags(d)).tocsr()
        M.sort_indices()
        assert np.array_equal(M.indices, A.colidx)
        return S.CSR(A.rowptr.copy(), A.colidx.copy(), M.data.copy(), A.nrows)
    if grid[2] > 1:
        return S.AssembleOperator_Laplace3D(*grid, kappa=1.0 + rng.random((grid[0] - 1) * (grid[1] - 1) * (grid[2] - 1)))[0]
    return S.AssembleOperator_Laplace(grid[0], grid[1], kappa=1.0 + rng.random((grid[0] - 1) * (grid[1] - 1)))[0]


@pytest.mark.parametrize("name", ["12x10any", "33x9", "6x4x3any", "five17x9"])
def test_refresh_gives_the_bytes_of_a_build(name):
    A0, A1 = operator(name), _scaled(name)
    assert np.array_equal(A0.colidx, A1.colidx) and not np.array_equal(A0.val, A1.val)
    h = build(name, galerkin="stencil")
    b0 = all_bytes(h)
    h.refresh(A0.val)
    assert all_bytes(h) == b0, "a refresh with unchanged values changed a byte"
    h.refresh(A1.val)
    fresh = build(name, A=A1, galerkin="stencil")
    b1 = all_bytes(h)
    assert b1 == all_bytes(fresh) and b1[0] != b0[0]
    assert b1[1] == b0[1], "the refresh changed P"
    assert h.info()["galerkin"] == S.AMG_GALERKIN_STENCIL
    h.close(), fresh.close()


# ---- 7. the refusals ---------------------------------------------------------------------------------------------------
def _far_pair():
    """five_point(17, 9) plus one symmetric pair of entries between nodes two apart in x (rows 20 and 22)"""
    A = operator("five17x9")
    M = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows)).tolil()
    M[20, 22] = M[22, 20] = -0.01
    M = M.tocsr()
    M.sort_indices()
    return S.CSR(M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.copy(), A.nrows)


def test_an_entry_outside_the_stencil_is_refused_by_name():
    A = _far_pair()
    with pytest.raises(SpkError) as e:
        build("five17x9", A=A, galerkin="stencil")
    assert e.value.code == SPK_ERR_UNSUPPORTED
    assert "row 20, column 22" in str(e.value) and "-spk_mg_galerkin products" in str(e.value), str(e.value)
    h = build("five17x9", A=A, galerkin="products")
    assert h.info()["levels"] >= 3 and h.info()["galerkin"] == 0
    h.close()


def test_option_values():
    with pytest.raises(SpkError) as e:
        build("5x5", galerkin=7)
    assert e.value.code == SPK_ERR_ARG and "galerkin" in str(e.value)
    assert S.solver.amg_opts_dict(S.amg_opts(galerkin="stencil"))["galerkin"] == S.AMG_GALERKIN_STENCIL
    assert S.solver.amg_opts_dict(S.amg_opts(galerkin=1))["galerkin"] == 1
    # under aggregation the field is not read
    A = S.AssembleOperator_Laplace(17, 17)[0]
    h0, h1, h2 = S.AmgHierarchy(A), S.AmgHierarchy(A, galerkin="stencil"), S.AmgHierarchy(A, galerkin=7)
    assert h1.info()["galerkin"] == 0 and h1.info()["coarsening"] == S.AMG_COARSEN_AGGREGATION
    assert all_bytes(h0)[0] == all_bytes(h1)[0] == all_bytes(h2)[0]
    for h in (h0, h1, h2):
        h.close()


@pytest.mark.parametrize("prefix", ["", "-fieldsplit_0_"])
def test_facade_reads_back_the_option(prefix):
    k = S.KSP()
    pc = ["-pc_type", "mg"] if not prefix else ["-pc_type", "fieldsplit", "-fieldsplit_0_ksp_type", "preonly", "-fieldsplit_0_pc_type", "mg"]
    key = prefix + "spk_mg_galerkin" if prefix else "-spk_mg_galerkin"
    k.setFromOptions(["-ksp_type", "fgmres"] + pc)
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["galerkin"] == S.AMG_GALERKIN_PRODUCTS
    k.setFromOptions([key, "stencil"])
    got, sel = k.getAMGOptions(fieldsplit0=bool(prefix))
    other, osel = k.getAMGOptions(fieldsplit0=not prefix)
    assert sel and not osel and got["galerkin"] == S.AMG_GALERKIN_STENCIL and other["galerkin"] == S.AMG_GALERKIN_PRODUCTS
    k.setFromOptions([prefix + "pc_mg_galerkin" if prefix else "-pc_mg_galerkin", "both"])   # PETSc's option keeps its meaning
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["galerkin"] == S.AMG_GALERKIN_STENCIL
    k.setFromOptions([key, "products"])
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["galerkin"] == S.AMG_GALERKIN_PRODUCTS
    for opts, code, words in (([key, "gather"], SPK_ERR_UNSUPPORTED, "products | stencil"), ([key, "1"], SPK_ERR_UNSUPPORTED, "products | stencil"),
                              ([key], SPK_ERR_ARG, "")):
        with pytest.raises(SpkError) as e:
            k.setFromOptions(opts)
        assert e.value.code == code and words in str(e.value), opts
    k.destroy()
    k = S.KSP()   # without mg selected: read and not used
    k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "gamg", "-spk_mg_galerkin", "stencil"])
    got, sel = k.getAMGOptions()
    assert sel and got["coarsening"] == S.AMG_COARSEN_AGGREGATION and got["galerkin"] == S.AMG_GALERKIN_STENCIL
    k.destroy()


# ---- 8. the defaults ---------------------------------------------------------------------------------------------------
def test_the_default_is_the_products_route_byte_for_byte(built):
    name, _, g = built
    assert S.solver.amg_opts_dict(S.amg_opts())["galerkin"] == S.AMG_GALERKIN_PRODUCTS == 0
    p = build(name, galerkin="products")
    assert g.info()["galerkin"] == 0 and all_bytes(g) == all_bytes(p)
    p.close()


# ---- 9. the stand-alone host program under the sanitizers --------------------------------------------------------------
def test_galerkin_stencil_host_check_program(tmp_path):
    exe = tmp_path / "galerkin_stencil_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(CSRC, "spk_host.cpp"), os.path.join(CSRC, "spk_galerkin_host.cpp"),
                           os.path.join(ROOT, "tests", "host", "galerkin_stencil_check.cpp"),
                           "-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all galerkin stencil host checks passed" in out.stdout


# ---- 10. the kernels' resources ----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_stencil_kernels_have_no_scratch_and_no_spill(tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spk_k_amg_setup.hip"), "-o", str(tmp_path / "amgs.o")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if re.match(r"_ZN3spk1k\d+amgs_galerkin_stencil", b)]
    names = [b.split()[0] for b in blocks]
    for bs in (1, 2, 3):   # the gather and the symmetrisation of every node size, and the level-0 check
        assert sum(f"stencil_kernelILi{bs}E" in n for n in names) == 1 and sum(f"stencil_sym_kernelILi{bs}E" in n for n in names) == 1, names
    assert sum("stencil_check_kernel" in n for n in names) == 1 and len(blocks) == 7, names
    for b in blocks:
        field = lambda pat: int(re.search(pat + r": (\d+)", b).group(1))
        print("%s: vgpr %d sgpr %d lds %d waves/SIMD %d" % (b.split()[0], field("VGPRs"), field("SGPRs"), field(r"LDS Size \[bytes/block\]"),
                                                            field(r"Occupancy \[waves/SIMD\]")))
        assert field(r"ScratchSize \[bytes/lane\]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, b.split()[0]
