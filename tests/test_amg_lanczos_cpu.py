"""-spk_amg_lanczos resident without a GPU (include/spk.h, SPK_AMG_LANCZOS_RESIDENT; csrc/spk_lanczos_core.hpp): the option's
values and default, the host builder taking and not reading it, the facade reading it back under both prefixes with its
refusals, the stand-alone host program under the sanitizers -- the state machine of the resident route against the
push_back / break loop of the stepwise one, byte for byte -- and the new kernels' resource remarks."""
import os
import re
import subprocess

import pytest

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError
from test_mg_galerkin_cpu import CSRC, HIPCC, ROOT, all_bytes, build

SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6


# ---- 1. values and default ---------------------------------------------------------------------------------------------
def test_option_values_and_default():
    assert S.AMG_LANCZOS_STEPWISE == 0 and S.AMG_LANCZOS_RESIDENT == 1
    assert S.solver.amg_opts_dict(S.amg_opts())["lanczos"] == 0
    assert S.solver.amg_opts_dict(S.amg_opts(lanczos="resident"))["lanczos"] == S.AMG_LANCZOS_RESIDENT
    assert S.solver.amg_opts_dict(S.amg_opts(lanczos="stepwise"))["lanczos"] == S.AMG_LANCZOS_STEPWISE
    assert S.solver.amg_opts_dict(S.amg_opts(lanczos=1))["lanczos"] == 1
    with pytest.raises(KeyError):
        S.amg_opts(lanczos="fused")
    A = S.AssembleOperator_Laplace(17, 17)[0]
    for bad in (7, -1):
        with pytest.raises(SpkError) as e:
            build("5x5", lanczos=bad)
        assert e.value.code == SPK_ERR_ARG and "lanczos" in str(e.value), str(e.value)
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A, lanczos=bad)
        assert e.value.code == SPK_ERR_ARG and "lanczos" in str(e.value), str(e.value)


@pytest.mark.parametrize("name", ["33x9", "12x10any"])
def test_host_builder_takes_the_option_and_does_not_read_it(name):
    """the host builder range-checks the field and otherwise ignores it, as it does `setup`: resident with the default
    setup (host) is no refusal there, and the hierarchy is the default's to the byte"""
    r, d = build(name, lanczos="resident"), build(name)
    assert all_bytes(r) == all_bytes(d)
    assert r.info()["lanczos"] == 0 and r.info()["ritz_readbacks"] == 0 and d.info()["ritz_readbacks"] == 0
    r.close(), d.close()
    A = S.AssembleOperator_Laplace(17, 17)[0]
    r, d = S.AmgHierarchy(A, lanczos="resident", setup="device"), S.AmgHierarchy(A)
    assert all_bytes(r) == all_bytes(d) and r.info()["ritz_readbacks"] == 0
    r.close(), d.close()


def test_the_gpu_cases_have_the_levels_they_are_chosen_for():
    """the hierarchies of tests/test_gpu_amg_lanczos.py on the host builder: every case coarsens, and its first levels
    have the rows its comment names (a ragged last workgroup at 1122 rows, many workgroups at 33 282, kk = 18 at 18)"""
    from test_gpu_amg_lanczos import CASES, operator as gpu_operator
    for name, (_, amg, rows) in CASES.items():
        h = S.AmgHierarchy(gpu_operator(name), **amg)
        info = h.info()
        h.close()
        print(name, info["rows"])
        assert info["levels"] >= 2 and info["rows"][:len(rows)] == rows, (name, info["rows"])


# ---- 2. the facade -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["", "-fieldsplit_0_"])
def test_facade_reads_back_the_option(prefix):
    k = S.KSP()
    pc = ["-pc_type", "mg"] if not prefix else ["-pc_type", "fieldsplit", "-fieldsplit_0_ksp_type", "preonly", "-fieldsplit_0_pc_type", "mg"]
    key = prefix + "spk_amg_lanczos" if prefix else "-spk_amg_lanczos"
    k.setFromOptions(["-ksp_type", "fgmres"] + pc)
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["lanczos"] == S.AMG_LANCZOS_STEPWISE
    k.setFromOptions([key, "resident"])
    got, sel = k.getAMGOptions(fieldsplit0=bool(prefix))
    other, osel = k.getAMGOptions(fieldsplit0=not prefix)
    assert sel and not osel and got["lanczos"] == S.AMG_LANCZOS_RESIDENT and other["lanczos"] == S.AMG_LANCZOS_STEPWISE
    assert got["setup"] == S.AMG_SETUP_HOST   # the option sets nothing else
    k.setFromOptions([key, "stepwise"])
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["lanczos"] == S.AMG_LANCZOS_STEPWISE
    for opts, code, words in (([key, "device"], SPK_ERR_UNSUPPORTED, "stepwise | resident"), ([key, "1"], SPK_ERR_UNSUPPORTED, "stepwise | resident"),
                              ([key], SPK_ERR_ARG, "")):
        with pytest.raises(SpkError) as e:
            k.setFromOptions(opts)
        assert e.value.code == code and words in str(e.value), opts
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["lanczos"] == S.AMG_LANCZOS_STEPWISE   # a refusal changes nothing
    k.destroy()
    k = S.KSP()   # without multigrid selected: read and not used
    k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "jacobi", "-spk_amg_lanczos", "resident"])
    got, sel = k.getAMGOptions()
    assert not sel and got["lanczos"] == S.AMG_LANCZOS_RESIDENT
    k.destroy()


# ---- 3. the stand-alone host program under the sanitizers --------------------------------------------------------------
def test_lanczos_core_host_check_program(tmp_path):
    exe = tmp_path / "lanczos_core_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "lanczos_core_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all lanczos core checks passed" in out.stdout
    steps = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"^case (.+?) +n +\d+ kk +\d+ steps +(\d+)", out.stdout, re.M)}
    assert steps == {"dense40": 30, "dense18": 18, "diagonal": 1, "three eigenvalues": 3, "nan at step 2": 30, "one row": 1}, out.stdout


# ---- 4. the kernels' resources -----------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_resident_kernels_have_no_scratch_and_no_spill(tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spk_k_amg_setup.hip"), "-o", str(tmp_path / "setup.o")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]
              if re.match(r"_ZN3spk1k\d+amgs_lz_(init|scale|dot|update)_resident_kernel", b)]
    names = [b.split()[0] for b in blocks]
    for which in ("init", "scale", "dot", "update"):
        assert sum(f"amgs_lz_{which}_resident_kernel" in n for n in names) == 1, names
    assert len(blocks) == 4, names
    for b in blocks:
        field = lambda pat: int(re.search(pat + r": (\d+)", b).group(1))
        print("%s: vgpr %d sgpr %d static lds %d waves/SIMD %d" % (b.split()[0], field("VGPRs"), field("SGPRs"), field(r"LDS Size \[bytes/block\]"),
                                                                   field(r"Occupancy \[waves/SIMD\]")))
        assert field(r"ScratchSize \[bytes/lane\]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, b.split()[0]
