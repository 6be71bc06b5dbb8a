"""-spk_mg_operator stencil without a GPU (include/spk.h, SPK_AMG_OPERATOR_STENCIL; csrc/spk_stencil_op_core.hpp): the option's
values and default, the facade reading it back under both prefixes, the refusals by name, the hierarchy's bytes (the option
steers the application, not the hierarchy), the stand-alone host program under the sanitizers -- the core function of a row
against a plain CSR loop, byte for byte -- and the kernels' resource remarks."""
import os
import re
import subprocess

import pytest

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError
from test_mg_galerkin_cpu import CSRC, HIPCC, ROOT, all_bytes, build, operator

SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6


# ---- 1. values and default ---------------------------------------------------------------------------------------------
def test_option_values_and_default():
    assert S.AMG_OPERATOR_CSR == 0 and S.AMG_OPERATOR_STENCIL == 1
    d = S.solver.amg_opts_dict(S.amg_opts())
    assert d["op"] == 0 and d["operator"] == 0
    assert S.solver.amg_opts_dict(S.amg_opts(operator="stencil"))["op"] == S.AMG_OPERATOR_STENCIL
    assert S.solver.amg_opts_dict(S.amg_opts(operator="csr"))["op"] == S.AMG_OPERATOR_CSR
    assert S.solver.amg_opts_dict(S.amg_opts(operator=1))["operator"] == 1
    with pytest.raises(KeyError):
        S.amg_opts(operator="dense")
    for kw in (dict(operator=7), dict(operator=-1), dict(operator=2, galerkin="stencil")):
        with pytest.raises(SpkError) as e:
            build("5x5", **kw)
        assert e.value.code == SPK_ERR_ARG and "op " in str(e.value), str(e.value)
    h = build("5x5")
    assert h.info()["operator"] == S.AMG_OPERATOR_CSR
    h.close()


# ---- 2. the facade -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["", "-fieldsplit_0_"])
def test_facade_reads_back_the_option(prefix):
    k = S.KSP()
    pc = ["-pc_type", "mg"] if not prefix else ["-pc_type", "fieldsplit", "-fieldsplit_0_ksp_type", "preonly", "-fieldsplit_0_pc_type", "mg"]
    key = prefix + "spk_mg_operator" if prefix else "-spk_mg_operator"
    k.setFromOptions(["-ksp_type", "fgmres"] + pc)
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["operator"] == S.AMG_OPERATOR_CSR
    k.setFromOptions([key, "stencil"])
    got, sel = k.getAMGOptions(fieldsplit0=bool(prefix))
    other, osel = k.getAMGOptions(fieldsplit0=not prefix)
    assert sel and not osel and got["operator"] == S.AMG_OPERATOR_STENCIL and other["operator"] == S.AMG_OPERATOR_CSR
    assert got["galerkin"] == S.AMG_GALERKIN_PRODUCTS   # the option sets nothing else
    k.setFromOptions([key, "csr"])
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["operator"] == S.AMG_OPERATOR_CSR
    for opts, code, words in (([key, "ell"], SPK_ERR_UNSUPPORTED, "csr | stencil"), ([key, "1"], SPK_ERR_UNSUPPORTED, "csr | stencil"),
                              ([key], SPK_ERR_ARG, "")):
        with pytest.raises(SpkError) as e:
            k.setFromOptions(opts)
        assert e.value.code == code and words in str(e.value), opts
    k.destroy()
    k = S.KSP()   # without multigrid selected: read and not used
    k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "jacobi", "-spk_mg_operator", "stencil"])
    got, sel = k.getAMGOptions()
    assert not sel and got["operator"] == S.AMG_OPERATOR_STENCIL
    k.destroy()


# ---- 3. the refusals ---------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_missing():
    with pytest.raises(SpkError) as e:   # the generic products keep no closed form
        build("33x9", operator="stencil", galerkin="products")
    assert e.value.code == SPK_ERR_UNSUPPORTED and "-spk_mg_galerkin stencil" in str(e.value), str(e.value)
    with pytest.raises(SpkError) as e:   # ... which is the default
        build("33x9", operator="stencil")
    assert e.value.code == SPK_ERR_UNSUPPORTED and "-spk_mg_galerkin stencil" in str(e.value), str(e.value)
    A = S.AssembleOperator_Laplace(17, 17)[0]
    for kw in (dict(operator="stencil"), dict(operator="stencil", galerkin="stencil")):   # smoothed aggregation
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A, **kw)
        assert e.value.code == SPK_ERR_UNSUPPORTED and "-pc_type mg" in str(e.value), str(e.value)
    # the library is usable afterwards
    h = S.AmgHierarchy(A)
    assert h.info()["levels"] >= 2 and h.info()["operator"] == 0
    h.close()
    h = build("33x9", operator="stencil", galerkin="stencil")
    assert h.info()["operator"] == S.AMG_OPERATOR_STENCIL and h.info()["galerkin"] == S.AMG_GALERKIN_STENCIL
    h.close()


# ---- 4. the hierarchy's bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33x9", "12x10any", "6x4x3any", "five17x9"])
def test_hierarchy_bytes_are_those_of_csr(name):
    s, c = build(name, galerkin="stencil", operator="stencil"), build(name, galerkin="stencil", operator="csr")
    assert (s.info()["operator"], c.info()["operator"]) == (1, 0)
    assert all_bytes(s) == all_bytes(c)
    A = operator(name)
    s.refresh(A.val)   # the refresh keeps the option and the bytes
    assert s.info()["operator"] == 1 and all_bytes(s) == all_bytes(c)
    s.close(), c.close()


# ---- 5. the stand-alone host program under the sanitizers --------------------------------------------------------------
def test_stencil_op_host_check_program(tmp_path):
    exe = tmp_path / "stencil_op_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "stencil_op_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all stencil operator host checks passed" in out.stdout
    assert len(re.findall(r"^grid ", out.stdout, re.M)) == 14   # 4 flat grids x 3 node sizes, 2 in 3-D


# ---- 6. the kernels' resources -----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_operator_kernels_have_no_scratch_and_no_spill(tmp_path):
    """the LDS of amg_stencil_kernel is dynamic (the remark prints 0): the launch sizes it, at most 32 KiB in 2-D"""
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spk_k_amg.hip"), "-o", str(tmp_path / "amg.o")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if re.match(r"_ZN3spk1k\d+amg_(stencil_tail|stencil|tail)_kernel", b)]
    names = [b.split()[0] for b in blocks]
    for bs in (1, 2, 3):
        for mode in (0, 1):
            assert sum(f"amg_stencil_kernelILi{bs}ELi{mode}E" in n for n in names) == 1, names
    assert sum("amg_tail_kernel" in n for n in names) == 1 and sum("amg_stencil_tail_kernel" in n for n in names) == 1, names
    assert len(blocks) == 8, names   # six launches, the tail with the route and the tail without it
    for b in blocks:
        field = lambda pat: int(re.search(pat + r": (\d+)", b).group(1))
        print("%s: vgpr %d sgpr %d static lds %d waves/SIMD %d" % (b.split()[0], field("VGPRs"), field("SGPRs"), field(r"LDS Size \[bytes/block\]"),
                                                                   field(r"Occupancy \[waves/SIMD\]")))
        assert field(r"ScratchSize \[bytes/lane\]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, b.split()[0]
