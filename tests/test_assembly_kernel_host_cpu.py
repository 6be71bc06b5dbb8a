"""The device assembly kernels without a GPU.  Their phases are plain functions of (thread, workgroup) in
csrc/spk_assembly_core.hpp; tests/host/assembly_kernel_check.cpp runs them on the CPU -- every workgroup of the launch
grid, phase by phase, thread 0..255 in turn, outputs and LDS arrays allocated at exactly their sizes -- and compares
rowptr / colidx / val / f with the host assembler byte for byte.  Compiled with g++ and the sanitizers together with
spk_assembly.cpp, run as a plain process.

Cases: the grids and slabs of the GPU tests (test_gpu_assembly.py, test_gpu_assembly3d.py) -- the smallest shapes that
cross a strip seam, leave a tail strip and take the workgroup index through every (j, k) -- each with and without
boundary conditions, kappa absent and random (fixed seed)."""
import os
import re
import shutil
import subprocess

import pytest

import test_assembly3d_cpu as cpu3
import test_assembly_kappa_cpu as cpu2
import test_gpu_assembly as gpu2
import test_gpu_assembly3d as gpu3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def cases(tmp_path):
    lines = []
    for mx, my in gpu2.GRIDS:
        kfile = tmp_path / f"kappa_{mx}_{my}.bin"
        cpu2.random_kappa(mx, my).astype("<f8").tofile(kfile)
        for rb, re_ in gpu2.slabs(mx, my):
            for bc in (0, 1):
                for k in ("-", kfile):
                    lines.append(f"2 {mx} {my} 0 {rb} {re_} {bc} {k}")
    for mx, my, mz in gpu3.GRIDS:
        kfile = tmp_path / f"kappa_{mx}_{my}_{mz}.bin"
        cpu3.random_kappa(mx, my, mz).astype("<f8").tofile(kfile)
        for rb, re_ in gpu3.slabs(mx, my, mz):
            for bc in (0, 1):
                for k in ("-", kfile):
                    lines.append(f"3 {mx} {my} {mz} {rb} {re_} {bc} {k}")
    return lines


def test_kernel_phases_on_the_cpu_reproduce_the_host_assembler(tmp_path):
    exe = tmp_path / "assembly_kernel_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, os.path.join(CSRC, "spk_assembly.cpp"),
                           os.path.join(ROOT, "tests", "host", "assembly_kernel_check.cpp"), "-o", str(exe), "-lpthread"])
    lines = cases(tmp_path)
    assert len(lines) >= 4 * (3 * len(gpu2.GRIDS) + 3 * len(gpu3.GRIDS))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert f"{len(lines)} cases, 0 failed" in out.stdout
    assert "all assembly kernel host checks passed" in out.stdout


def test_core_header_includes_nothing_from_rocm():
    """spk_assembly_core.hpp: the standard library only (the compile above has no ROCm include path; this names the rule)"""
    src = open(os.path.join(CSRC, "spk_assembly_core.hpp")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs and all(i.startswith("<") and "hip" not in i and "rccl" not in i for i in incs), incs


# ---- the 2-D kernel's build-time shape (spk_k_assembly.hip), from the compiler's resource remark for gfx950; the 3-D
# kernel's is in test_assembly3d_cpu.py
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_resources(tmp_path):
    """no scratch, no spill, 57 552 B of LDS = (2 x 33) x (64 Ke + 8 Fe + 4 x 9 gradients + 1 kappa)
    doubles, and registers for the two waves per SIMD that the LDS allows (two workgroups per CU)."""
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spk_k_assembly.hip"), "-o", str(tmp_path / "k.o")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    found = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        if "assemble_laplace_kernel" in block.split("\n", 1)[0]:
            found = {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in cpu3.FIELDS.items()}
    print(found)
    assert found, p.stderr[-2000:]
    assert found["scratch"] == 0 and found["vspill"] == 0
    assert found["lds"] == 57552
    assert found["waves"] >= 2
