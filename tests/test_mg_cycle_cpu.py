"""The multigrid cycle (-spk_mg_cycle v|w) and the fused coarse tail (-spk_mg_tail, -spk_mg_tail_rows) without a GPU: the
three options through every layer, the step list of one cycle against the textbook recursion, the rule that picks the
tail's first level on host-built hierarchies, a numpy restatement of the cycle (cycle_ref, which test_gpu_mg_cycle holds
the device to) with its symmetry and the W-against-V iteration counts of numpy PCG, the host-pure code under the
sanitizers as a plain process, and the tail kernel's build-time resources."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError
from test_amg_cpu import hierarchy_mats, vcycle_ref

SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PRE0, PRE, DOWN, COARSE, UP, POST = range(6)


# ---- the numpy restatement ----------------------------------------------------------------------------------------------
def cycle_ref(A, P, Ci, lam, b, gamma=1, smoother="chebyshev", smooth_its=2, esteig=(0, 0.1, 0, 1.1), richardson_scale=1.0):
    """One cycle as the step list orders it: gamma = 1 the V-cycle, gamma = 2 the W-cycle (a second visit of level l + 1,
    from its own iterate, unless l + 1 is the coarsest).  The smoother is vcycle_ref's: nu steps
    y+ = y + alpha D^-1 (b - A y) + beta (y - y-), Chebyshev coefficients of Saad Alg. 12.1 over [b lmax, d lmax]."""
    L = len(A)
    dinv = [1.0 / np.where(a.diagonal() == 0.0, 1.0, a.diagonal()) for a in A]
    coef = []
    for l in range(L - 1):
        if smoother == "chebyshev":
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
        else:
            al, be = [richardson_scale] * smooth_its, [0.0] * smooth_its
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

    def rec(l, bb, y):
        if l == L - 1:
            return Ci @ bb
        y = smooth(l, bb, y)                      # PRE0 (y None) or PRE
        r = P[l].T @ (bb - A[l] @ y)              # DOWN
        e = rec(l + 1, r, None)
        if gamma == 2 and l + 1 < L - 1:
            e = rec(l + 1, r, e)
        return smooth(l, bb, y + P[l] @ e)        # UP, POST

    return rec(0, np.asarray(b, np.float64), None)


def pcg_its(Asp, b, M, rtol=1e-8, max_it=200):
    """iterations of textbook preconditioned CG until ||b - A x|| <= rtol ||b||"""
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    p = z.copy()
    rz = r @ z
    nb = np.linalg.norm(b)
    for it in range(1, max_it + 1):
        Ap = Asp @ p
        a = rz / (p @ Ap)
        x += a * p
        r -= a * Ap
        if np.linalg.norm(r) <= rtol * nb:
            return it
        z = M(r)
        rz, rz0 = r @ z, rz
        p = z + (rz / rz0) * p
    return max_it + 1


def steps_ref(L, w):
    """the definition of include/spk.h, word for word"""
    out = []

    def cycle(l, fresh):
        if l == L - 1:
            out.append((COARSE, l))
            return
        out.extend([(PRE0 if fresh else PRE, l), (DOWN, l)])
        cycle(l + 1, True)
        if w and l + 1 < L - 1:
            cycle(l + 1, False)
        out.extend([(UP, l), (POST, l)])

    cycle(0, True)
    return out


HIER = {"mg33": (lambda: S.AssembleOperator_Laplace(33, 33)[0], dict(coarsening="grid", grid=(33, 33))),
        "mg33_200": (lambda: S.AssembleOperator_Laplace(33, 33)[0], dict(coarsening="grid", grid=(33, 33), coarse_eq_limit=200)),
        "gamg32": (lambda: S.AssembleOperator_Laplace(32)[0], {}),
        "gamg64": (lambda: S.AssembleOperator_Laplace(64)[0], {})}


@functools.lru_cache(maxsize=None)
def _operator(name):
    return HIER[name][0]()


@functools.lru_cache(maxsize=None)
def _mats(name):
    """(scipy A_0, A_l, P_l, coarse inverse, lambda_max) of a host-built hierarchy; built once, never changed"""
    h = S.AmgHierarchy(_operator(name), **HIER[name][1])
    info = h.info()
    A, P, Ci = hierarchy_mats(h.matrix, info)
    h.close()
    return A, P, Ci, info["lambda_max"]


def _info(name, **kw):
    h = S.AmgHierarchy(_operator(name), **dict(HIER[name][1], **kw))
    info = h.info()
    h.close()
    return info


# ---- options ---------------------------------------------------------------------------------------------------------------
def test_defaults_and_round_trip():
    o = S.amg_opts()
    assert (o.cycle, o.tail, o.tail_rows) == (0, 0, 0)
    assert (S.AMG_CYCLE_V, S.AMG_CYCLE_W, S.AMG_TAIL_AUTO, S.AMG_TAIL_LAUNCHES, S.AMG_TAIL_FUSED) == (0, 1, 0, 1, 2)
    from saddle_point_petsc_amd.solver import amg_opts_dict
    for cyc, ci in (("v", 0), ("w", 1), (1, 1)):
        for tail, ti in (("auto", 0), ("launches", 1), ("fused", 2), (2, 2)):
            d = amg_opts_dict(S.amg_opts(cycle=cyc, tail=tail, tail_rows=600))
            assert (d["cycle"], d["tail"], d["tail_rows"]) == (ci, ti, 600)
    with pytest.raises(KeyError):
        S.amg_opts(cycle="f")
    with pytest.raises(KeyError):
        S.amg_opts(tail="kernel")


@pytest.mark.parametrize("kw,word", [(dict(cycle=2), "cycle 2"), (dict(tail=3), "tail 3"), (dict(tail_rows=-1), "tail_rows -1"),
                                     (dict(cycle=-1), "cycle -1")])
def test_host_builder_refuses_unknown_values(kw, word):
    with pytest.raises(SpkError) as e:
        S.AmgHierarchy(_operator("gamg32"), **kw)
    assert e.value.code == SPK_ERR_ARG and word in str(e.value)


def test_facade_reads_the_options():
    k = S.KSP()
    k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "mg", "-spk_mg_cycle", "w", "-fieldsplit_0_spk_mg_tail", "fused",
                      "-spk_mg_tail_rows", "600", "-pc_mg_cycle_type", "v"])
    plain, sel = k.getAMGOptions(False)
    split, _ = k.getAMGOptions(True)
    assert sel and (plain["cycle"], plain["tail"], plain["tail_rows"]) == (S.AMG_CYCLE_W, S.AMG_TAIL_AUTO, 600)
    assert (split["cycle"], split["tail"], split["tail_rows"]) == (S.AMG_CYCLE_V, S.AMG_TAIL_FUSED, 0)
    k.setFromOptions(["-fieldsplit_0_spk_mg_cycle", "w", "-spk_mg_tail", "launches", "-spk_mg_cycle", "v"])
    plain, _ = k.getAMGOptions(False)
    split, _ = k.getAMGOptions(True)
    assert (plain["cycle"], plain["tail"], split["cycle"]) == (S.AMG_CYCLE_V, S.AMG_TAIL_LAUNCHES, S.AMG_CYCLE_W)
    k.destroy()


@pytest.mark.parametrize("opts,code,word", [
    (["-spk_mg_cycle"], SPK_ERR_ARG, "needs"),
    (["-spk_mg_cycle", "f"], SPK_ERR_UNSUPPORTED, "v | w"),
    (["-fieldsplit_0_spk_mg_cycle", "full"], SPK_ERR_UNSUPPORTED, "v | w"),
    (["-spk_mg_tail"], SPK_ERR_ARG, "needs"),
    (["-spk_mg_tail", "kernel"], SPK_ERR_UNSUPPORTED, "auto | launches | fused"),
    (["-spk_mg_tail_rows"], SPK_ERR_ARG, "needs"),
    (["-spk_mg_tail_rows", "many"], SPK_ERR_ARG, "needs"),
    (["-spk_mg_tail_rows", "-3"], SPK_ERR_ARG, "needs"),
    (["-pc_mg_cycle_type", "w"], SPK_ERR_UNSUPPORTED, "-spk_mg_cycle w"),
    (["-fieldsplit_0_pc_mg_cycle_type", "w"], SPK_ERR_UNSUPPORTED, "-fieldsplit_0_spk_mg_cycle w"),
])
def test_facade_refuses_missing_and_unknown_values(opts, code, word):
    k = S.KSP()
    with pytest.raises(SpkError) as e:
        k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "mg"] + opts)
    assert e.value.code == code and word in str(e.value), str(e.value)
    k.destroy()


# ---- the step list -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", range(1, 9))
def test_step_list_is_the_recursion(L):
    for cyc in ("v", "w"):
        st = S.amg_cycle_steps(L, cyc)
        assert st == steps_ref(L, cyc == "w"), (L, cyc)
        entered = [sum(1 for k, l in st if l == lev and k in (PRE0, PRE, COARSE)) for lev in range(L)]
        if cyc == "w":
            assert entered == [2 ** l for l in range(L - 1)] + [2 ** (L - 2) if L > 2 else 1], (L, entered)
        else:
            assert entered == [1] * L
            down = [s for l in range(L - 1) for s in ((PRE0, l), (DOWN, l))]
            up = [s for l in reversed(range(L - 1)) for s in ((UP, l), (POST, l))]
            assert st == down + [(COARSE, L - 1)] + up
    assert S.amg_cycle_steps(L, 0) == S.amg_cycle_steps(L, "v")


def test_step_hook_refuses_bad_arguments():
    for L, cyc in ((0, 0), (17, 0), (3, 2)):
        with pytest.raises(SpkError) as e:
            S.amg_cycle_steps(L, cyc)
        assert e.value.code == SPK_ERR_ARG


# ---- the tail rule -------------------------------------------------------------------------------------------------------
def _launches(cycle, t, L):
    if t < 0:
        return 0
    return 1 if cycle == "v" else 2 ** (t - 1) if t < L - 1 else 2 ** (L - 2)


@pytest.mark.parametrize("name,rows", [("mg33", [2178, 578, 162, 50]), ("mg33_200", [2178, 578, 162]), ("gamg32", None)])
def test_tail_rule_on_host_hierarchies(name, rows):
    base = _info(name)
    if rows is not None:
        assert base["rows"] == rows
    rows, L = base["rows"], base["levels"]
    assert L >= 3 and (base["cycle"], base["tail_first"], base["tail_launches"]) == (0, -1, 0)
    for cycle in ("v", "w"):
        auto = _info(name, cycle=cycle)
        assert auto["cycle"] == (cycle == "w") and auto["tail_first"] == (1 if cycle == "w" else -1)   # the default takes every level
        off = _info(name, cycle=cycle, tail="launches", tail_rows=rows[1])
        assert (off["tail_first"], off["tail_launches"]) == (-1, 0)
        for l in range(L):
            for tr, t in ((rows[l], max(l, 1)), (rows[l] - 1, l + 1 if l + 1 < L else -1)):
                got = _info(name, cycle=cycle, tail="fused", tail_rows=tr)
                assert got["tail_first"] == t, (name, cycle, tr, got["tail_first"], t)
                assert got["tail_launches"] == _launches(cycle, t, L), (name, cycle, tr, got["tail_launches"])
        one = _info(name, cycle=cycle, tail="fused", tail_rows=1)
        assert (one["tail_first"], one["tail_launches"]) == (-1, 0)


def test_one_level_has_no_tail():
    h = S.AmgHierarchy(S.AssembleOperator_Laplace(16)[0], max_levels=1, cycle="w", tail="fused")   # 512 rows, solved densely
    info = h.info()
    h.close()
    assert info["levels"] == 1 and (info["tail_first"], info["tail_launches"]) == (-1, 0)


def test_refresh_keeps_the_cycle_fields():
    A = _operator("mg33")
    h = S.AmgHierarchy(A, coarsening="grid", grid=(33, 33), cycle="w", tail_rows=162)
    before = h.info()
    h.refresh(2.0 * A.val)
    after = h.info()
    h.close()
    assert (before["cycle"], before["tail_first"], before["tail_launches"]) == (1, 2, 2)
    assert (after["cycle"], after["tail_first"], after["tail_launches"]) == (1, 2, 2)


# ---- the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mg33", "gamg32"])
def test_gamma_one_is_the_v_cycle(name):
    A, P, Ci, lam = _mats(name)
    x = np.random.default_rng(1).standard_normal(A[0].shape[0])
    for kw in (dict(), dict(smooth_its=3), dict(smoother="richardson", richardson_scale=0.6)):
        assert np.array_equal(cycle_ref(A, P, Ci, lam, x, 1, **kw), vcycle_ref(A, P, Ci, lam, x, **kw))


@pytest.mark.parametrize("name", ["mg33", "gamg64"])
def test_w_cycle_is_symmetric_and_needs_no_more_iterations(name):
    A, P, Ci, lam = _mats(name)
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal(A[0].shape[0]), rng.standard_normal(A[0].shape[0])
    assert len(A) >= 4   # a W-cycle differs from the V-cycle from four levels on (the coarsest is visited once per visit of L-2)
    Mx, My = cycle_ref(A, P, Ci, lam, x, 2), cycle_ref(A, P, Ci, lam, y, 2)
    assert not np.array_equal(Mx, cycle_ref(A, P, Ci, lam, x, 1))
    asym = abs(x @ My - y @ Mx) / max(abs(x @ My), abs(y @ Mx))
    print(f"{name}: x^T M y and y^T M x differ by {asym:.3e} relative (bound 1e-12)")
    assert asym <= 1e-12
    b = A[0] @ rng.standard_normal(A[0].shape[0])
    its = {g: pcg_its(A[0], b, lambda r, g=g: cycle_ref(A, P, Ci, lam, r, g)) for g in (1, 2)}
    print(f"{name}: PCG to 1e-8 in {its[1]} iterations with the V-cycle, {its[2]} with the W-cycle")
    assert its[2] <= its[1] <= 100


# ---- the host-pure code under the sanitizers -----------------------------------------------------------------------
def test_cycle_host_check_program(tmp_path):
    exe = tmp_path / "amg_cycle_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(CSRC, "spk_host.cpp"), os.path.join(ROOT, "tests", "host", "amg_cycle_check.cpp"),
                           "-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all multigrid cycle host checks passed" in out.stdout


# ---- the tail kernel's resources -------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tail_kernel_has_no_scratch_and_no_spill(tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spk_k_amg.hip"), "-o", str(tmp_path / "amg.o")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if re.match(r"_ZN3spk1k\d+amg_tail_kernel", b)]
    assert len(blocks) == 1, "amg_tail_kernel is missing from spk_k_amg.hip"

    def field(pat):
        return int(re.search(pat + r": (\d+)", blocks[0]).group(1))

    print("amg_tail_kernel: vgpr %d sgpr %d lds %d waves/SIMD %d" % (field("VGPRs"), field("SGPRs"), field(r"LDS Size \[bytes/block\]"),
                                                                     field(r"Occupancy \[waves/SIMD\]")))
    assert field(r"ScratchSize \[bytes/lane\]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
