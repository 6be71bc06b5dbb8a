"""The host-pure half of the operator set-up (csrc/spk_host.cpp: field layout of the dictionary, plane offsets, ghost
numbering, halo plan, windows and transpose of the constraint block) against brute-force references, without a GPU and
without ROCm: the sources are compiled with g++ and the sanitizers together with one self-checking program
(tests/host/setup_host_check.cpp), which runs as a plain process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")


def test_setup_host_steps(tmp_path):
    exe = tmp_path / "setup_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(CSRC, "spk_host.cpp"), os.path.join(ROOT, "tests", "host", "setup_host_check.cpp"),
                           "-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all set-up host checks passed" in out.stdout


def test_host_layer_includes_nothing_from_rocm():
    """spk_host.hpp / .cpp: the standard library and include/spk.h only (the compile above has no ROCm include path; this
    names the rule)."""
    for name in ("spk_host.hpp", "spk_host.cpp"):
        src = open(os.path.join(CSRC, name)).read()
        incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
        assert all(i.startswith("<") and "hip" not in i and "rccl" not in i or i in ('"spk_host.hpp"', '"../../include/spk.h"')
                   for i in incs), incs
