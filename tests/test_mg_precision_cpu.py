"""-spk_mg_precision single without a GPU (include/spk.h, SPK_AMG_PRECISION_SINGLE): the option's values and default, the
facade reading it back under both prefixes, every refusal by name, the hierarchy's bytes (the option steers the application,
not the hierarchy), the stand-alone host program under the sanitizers -- so_row on float against a plain float loop, byte for
byte, and the residues mod 4 of the workgroups' value ranges on the GPU test's shapes -- the numpy cycle with FP32 levels
(vcycle_ref_mixed, the reference of tests/test_gpu_mg_precision.py) inside a small FGMRES(30), and the resource remarks of the
FP32 kernels."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError
from test_gpu_mg_operator import SHAPES
from test_mg_cycle_cpu import cycle_ref
from test_mg_galerkin_cpu import CSRC, HIPCC, ROOT, all_bytes
from test_mg_sides_cpu import hierarchy_mats, vcycle_ref

SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6
F32 = np.float32
GPU_SHAPES = ["65x33", "66x34any", "33x9", "12x10any", "five17x9", "17x9x5", "6x4x3any", "4x4any"]


def route_kw(name, **kw):
    """the all-stencil route of SHAPES[name]: what precision='single' needs"""
    grid, bs, sides, _ = SHAPES[name]
    return dict(dict(coarsening="grid", grid=grid, sides=sides, block_size=bs, coarse_eq_limit=10, galerkin="stencil",
                     operator="stencil"), **kw)


@functools.lru_cache(maxsize=None)
def problem(name):
    return SHAPES[name][3]()


@functools.lru_cache(maxsize=None)
def host_hierarchy(name):
    """(info, (A, P, Ci)) of the host-built hierarchy: under galerkin='stencil' the device set-up's bytes"""
    h = S.AmgHierarchy(problem(name)[0], **route_kw(name))
    info = h.info()
    mats = hierarchy_mats(h.matrix, info)
    h.close()
    return info, mats


# ---- the numpy cycle with FP32 levels -----------------------------------------------------------------------------------
def vcycle_ref_mixed(A, P, Ci, lam, b, smooth_its=2, esteig=(0, 0.1, 0, 1.1), gamma=1, dinv=None):
    """vcycle_ref (test_mg_sides_cpu; gamma = 2: the W-cycle of test_mg_cycle_cpu.cycle_ref, a second visit of level l + 1
    from its own iterate unless it is the coarsest) with the levels >= 1 in numpy float32, as SPK_AMG_PRECISION_SINGLE states them: the
    values of A_l, D^-1 (the FP64 D^-1 rounded), the coefficients and the coarse inverse rounded once to float32, the vectors
    of the levels >= 1 float32 and every operation on them a float32 one; level 0 in float64; DOWN on level 0 computes
    R (b - A y) in float64 and rounds the result once, UP on level 0 widens e and adds in float64.  The transfer weights
    are powers of two, so P as float32 is exact.  dinv: a list per level of FP64 vectors in place of 1 / diag(A_l), rounded
    as that is (test_mg_varcoef_cpu.vcycle_with's argument: the mis-indexed cycles of test_mg_precision_varcoef_cpu.py)."""
    L = len(A)
    dt = lambda l: np.float64 if l == 0 else F32
    if dinv is None:
        dinv = [1.0 / np.where(a.diagonal() == 0.0, 1.0, a.diagonal()) for a in A]
    dinv = [np.asarray(d, np.float64).astype(dt(l)) for l, d in enumerate(dinv)]
    Al = [a.astype(dt(l)) for l, a in enumerate(A)]
    Pl = [p.astype(dt(l)) for l, p in enumerate(P)]
    Cl = Ci.astype(dt(L - 1))
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
        coef.append(([dt(l)(a) for a in al], [dt(l)(v) for v in be]))   # computed in float64, rounded once

    def smooth(l, bb, y):
        prev = None
        for al, be in zip(*coef[l]):
            if y is None:
                yn = al * (dinv[l] * bb)
            else:
                yn = y + al * (dinv[l] * (bb - Al[l] @ y))
                if be != 0.0:
                    yn = yn + be * (y - (prev if prev is not None else dt(l)(0.0)))
            assert yn.dtype == dt(l)
            prev, y = y, yn
        return y

    def rec(l, bb, y):
        assert bb.dtype == dt(l)
        if l == L - 1:
            return Cl @ bb
        y = smooth(l, bb, y)                                # PRE0 (y None) or PRE
        r = (Pl[l].T @ (bb - Al[l] @ y)).astype(F32)        # DOWN; level 0: the one rounding of the boundary
        e = rec(l + 1, r, None)
        if gamma == 2 and l + 1 < L - 1:
            e = rec(l + 1, r, e)
        return smooth(l, bb, y + Pl[l] @ e.astype(dt(l)))   # UP (level 0: e widened, exact), POST

    return rec(0, np.asarray(b, np.float64), None)


@functools.lru_cache(maxsize=None)
def cycle_difference(name, gamma=1, seed=3):
    """|| mixed - double || / || double || of one application of the two numpy cycles (gamma = 1: V, 2: W) on the host-built
    hierarchy"""
    info, mats = host_hierarchy(name)
    x = np.random.default_rng(seed).standard_normal(info["rows"][0])
    y64 = cycle_ref(*mats, info["lambda_max"], x, gamma)
    y32 = vcycle_ref_mixed(*mats, info["lambda_max"], x, gamma=gamma)
    return float(np.linalg.norm(y32 - y64) / np.linalg.norm(y64))


def fgmres_numpy(Aop, M, b, rtol=1e-8, restart=30, max_it=200):
    """flexible GMRES(restart), right-preconditioned by the callable M, from x = 0; returns (x, iterations)"""
    x = np.zeros_like(b)
    bn = np.linalg.norm(b)
    its = 0
    while its < max_it:
        r = b - Aop @ x
        beta = np.linalg.norm(r)
        if beta <= rtol * bn:
            break
        V, Z = [r / beta], []
        H = np.zeros((restart + 1, restart))
        g = np.zeros(restart + 1)
        g[0] = beta
        cs, sn = np.zeros(restart), np.zeros(restart)
        k = 0
        for k in range(restart):
            Z.append(M(V[k]))
            w = Aop @ Z[k]
            for i in range(k + 1):
                H[i, k] = V[i] @ w
                w = w - H[i, k] * V[i]
            H[k + 1, k] = np.linalg.norm(w)
            V.append(w / H[k + 1, k] if H[k + 1, k] > 0 else w)
            for i in range(k):
                H[i, k], H[i + 1, k] = cs[i] * H[i, k] + sn[i] * H[i + 1, k], -sn[i] * H[i, k] + cs[i] * H[i + 1, k]
            d = np.hypot(H[k, k], H[k + 1, k])
            cs[k], sn[k] = H[k, k] / d, H[k + 1, k] / d
            H[k, k], H[k + 1, k] = d, 0.0
            g[k + 1], g[k] = -sn[k] * g[k], cs[k] * g[k]
            its += 1
            if abs(g[k + 1]) <= rtol * bn or its >= max_it:
                break
        yk = np.linalg.solve(np.triu(H[:k + 1, :k + 1]), g[:k + 1])
        x = x + sum(c * z for c, z in zip(yk, Z))
    return x, its


# ---- 1. values and default ---------------------------------------------------------------------------------------------
def test_option_values_and_default():
    assert S.AMG_PRECISION_DOUBLE == 0 and S.AMG_PRECISION_SINGLE == 1
    assert S.solver.amg_opts_dict(S.amg_opts())["precision"] == 0
    assert S.solver.amg_opts_dict(S.amg_opts(precision="single"))["precision"] == S.AMG_PRECISION_SINGLE
    assert S.solver.amg_opts_dict(S.amg_opts(precision="double"))["precision"] == S.AMG_PRECISION_DOUBLE
    assert S.solver.amg_opts_dict(S.amg_opts(precision=1))["precision"] == 1
    with pytest.raises(KeyError):
        S.amg_opts(precision="half")
    A = problem("33x9")[0]
    for bad in (7, -1, 2):   # the host builder range-checks the field
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A, **route_kw("33x9", precision=bad))
        assert e.value.code == SPK_ERR_ARG and "precision" in str(e.value), str(e.value)


def test_host_builder_does_not_read_the_field():
    """as with lanczos: any route builds, the bytes are those of 'double', and a refresh keeps them"""
    A = problem("33x9")[0]
    grid, bs, sides, _ = SHAPES["33x9"]
    plain = dict(coarsening="grid", grid=grid, sides=sides, block_size=bs, coarse_eq_limit=10)
    for kw in (route_kw("33x9"), plain, dict(plain, transfer="stored")):
        s, d = S.AmgHierarchy(A, **dict(kw, precision="single")), S.AmgHierarchy(A, **kw)
        assert all_bytes(s) == all_bytes(d)
        s.refresh(A.val)
        assert all_bytes(s) == all_bytes(d)
        s.close(), d.close()
    g = S.AmgHierarchy(S.AssembleOperator_Laplace(17, 17)[0], precision="single")   # smoothed aggregation
    assert g.info()["levels"] >= 2
    g.close()


# ---- 2. the facade -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["", "-fieldsplit_0_"])
def test_facade_reads_back_the_option(prefix):
    k = S.KSP()
    pc = ["-pc_type", "mg"] if not prefix else ["-pc_type", "fieldsplit", "-fieldsplit_0_ksp_type", "preonly", "-fieldsplit_0_pc_type", "mg"]
    key = prefix + "spk_mg_precision" if prefix else "-spk_mg_precision"
    k.setFromOptions(["-ksp_type", "fgmres"] + pc)
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["precision"] == S.AMG_PRECISION_DOUBLE
    k.setFromOptions([key, "single"])
    got, sel = k.getAMGOptions(fieldsplit0=bool(prefix))
    other, osel = k.getAMGOptions(fieldsplit0=not prefix)
    assert sel and not osel and got["precision"] == S.AMG_PRECISION_SINGLE and other["precision"] == S.AMG_PRECISION_DOUBLE
    assert got["galerkin"] == S.AMG_GALERKIN_PRODUCTS and got["operator"] == S.AMG_OPERATOR_CSR   # the option sets nothing else
    k.setFromOptions([key, "double"])
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["precision"] == S.AMG_PRECISION_DOUBLE
    for opts, code, words in (([key, "half"], SPK_ERR_UNSUPPORTED, "double | single"), ([key, "1"], SPK_ERR_UNSUPPORTED, "double | single"),
                              ([key], SPK_ERR_ARG, "")):
        with pytest.raises(SpkError) as e:
            k.setFromOptions(opts)
        assert e.value.code == code and words in str(e.value), opts
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["precision"] == S.AMG_PRECISION_DOUBLE   # a refusal changes nothing
    k.destroy()
    k = S.KSP()   # without multigrid selected: read and not used
    k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "jacobi", "-spk_mg_precision", "single"])
    got, sel = k.getAMGOptions()
    assert not sel and got["precision"] == S.AMG_PRECISION_SINGLE
    k.destroy()


# ---- 3. the refusals (those of a live context: tests/test_gpu_mg_precision.py) ---------------------------------------------
@pytest.mark.parametrize("ksp", ["pipecg", "pipecgrr"])
def test_facade_refuses_pipelined_cg_at_setup(ksp):
    k = S.KSP()
    k.setFromOptions(["-ksp_type", ksp, "-pc_type", "mg", "-spk_mg_galerkin", "stencil", "-spk_mg_operator", "stencil",
                      "-spk_mg_precision", "single"])
    with pytest.raises(SpkError) as e:   # an option check: before the operators, without a GPU
        k.setUp()
    assert e.value.code == SPK_ERR_UNSUPPORTED and "-ksp_type fgmres" in str(e.value) and "-spk_mg_precision" in str(e.value), str(e.value)
    k.destroy()


# ---- 4. the stand-alone host program under the sanitizers --------------------------------------------------------------
def test_stencil_op_f32_host_check_program(tmp_path):
    """so_row on float equals a plain float loop in stored order on the levels the GPU test's hooks run on, and the begin and
    the end of the workgroups' value ranges take all four residues mod 4 over those shapes: every length of the peeled
    head and tail of the 16-byte staging occurs."""
    exe = tmp_path / "stencil_op_f32_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "stencil_op_f32_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)   # its own small grids
    assert out.returncode == 0 and "all FP32 stencil operator host checks passed" in out.stdout, out.stdout + out.stderr
    args = []
    for name in GPU_SHAPES:
        info, _ = host_hierarchy(name)
        for l in range(1, info["levels"] - 1):   # the levels the operator kernel runs on
            args += [str(info["block_size"])] + [str(d) for d in info["dims"][l]]
    out = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all FP32 stencil operator host checks passed" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    lines = re.findall(r"^grid .*begin residues mod 4:([ \d]*), end residues mod 4:([ \d]*)$", out.stdout, re.M)
    assert len(lines) == len(args) // 4 > 0
    begins = set(q for b, _ in lines for q in b.split())
    ends = set(q for _, e in lines for q in e.split())
    assert begins == {"0", "1", "2", "3"} and ends == {"0", "1", "2", "3"}, (begins, ends)


# ---- 5. the numpy mixed cycle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["65x33", "17x9x5"])
def test_mixed_cycle_in_fgmres(name):
    """FGMRES(30) to rtol 1e-8 on K = A with the numpy cycles: the iterations with FP32 levels are at most those of the FP64
    cycle + 1 (the project's parity bar for iteration counts; the model behind the option gave equal counts) and the true
    residual is at most 2e-8."""
    A, f = problem(name)
    Asp = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))
    info, mats = host_hierarchy(name)
    its = {}
    for label, cyc in (("double", vcycle_ref), ("mixed", vcycle_ref_mixed)):
        x, its[label] = fgmres_numpy(Asp, lambda r: cyc(*mats, info["lambda_max"], r), f)
        res = np.linalg.norm(f - Asp @ x) / np.linalg.norm(f)
        print(f"{name} {label}: {its[label]} iterations, true residual {res:.3e}")
        assert res <= 2e-8
    print(f"{name}: one application, mixed against double: {cycle_difference(name):.3e}")
    assert its["mixed"] <= its["double"] + 1, its


def test_mixed_cycle_differs_at_the_fp32_level():
    """the FP32 levels run in the reference: one application differs from the FP64 one by more than 1e-10 and by far less than
    1e-4 relative on every shape of the GPU test, under both cycles"""
    for name in GPU_SHAPES:
        for gamma in (1, 2):
            d = cycle_difference(name, gamma)
            print(f"{name} {'vw'[gamma - 1]}: {d:.3e}")
            assert 1e-10 < d < 1e-4, (name, gamma, d)
    info, mats = host_hierarchy("65x33")   # gamma = 1 is vcycle_ref's order of operations
    x = np.random.default_rng(1).standard_normal(info["rows"][0])
    assert np.array_equal(cycle_ref(*mats, info["lambda_max"], x, 1), vcycle_ref(*mats, info["lambda_max"], x))


# ---- 6. the kernels' resources -----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fp32_kernels_have_no_scratch_and_no_spill(tmp_path):
    """the FP32 launches (the six operator kernels, the zero-guess pass, the dense product, the float and the boundary
    transfers, the rounding pass) and the FP32 tail: no scratch, no spilled register"""
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spk_k_amg.hip"), "-o", str(tmp_path / "amg.o")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = {b.split()[0]: b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]}
    want = [f"amg_stencil_f32_kernelILi{bs}ELi{mode}E" for bs in (1, 2, 3) for mode in (0, 1)]
    want += ["amg_stencil_tail_f32_kernel", "amg_cheb_vec_kernelIfE", "amg_dense_kernelIfE", "amg_round_f32_kernel"]
    want += [f"amg_{k}_grid_kernelILi{bs}E{t}E" for bs in (1, 2, 3) for k, t in (("prolong", "ff"), ("prolong", "fd"), ("restrict", "ff"),
                                                                               ("restrict", "df"))]
    for w in want:
        hit = [n for n in blocks if w in n]
        assert len(hit) == 1, (w, hit)
        b = blocks[hit[0]]
        field = lambda pat: int(re.search(pat + r": (\d+)", b).group(1))
        print("%s: vgpr %d sgpr %d waves/SIMD %d" % (w, field("VGPRs"), field("SGPRs"), field(r"Occupancy \[waves/SIMD\]")))
        assert field(r"ScratchSize \[bytes/lane\]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, w
