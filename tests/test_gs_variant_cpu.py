"""Which instantiation form 7's fused Gram-Schmidt launch runs (csrc/spk_gs_launch.hpp: variant, grid, template arguments)
on the shapes of the GPU tests and at the edges of the rule, without a GPU and without ROCm (the header uses the standard
library only): compiled with g++ and the sanitizers into tests/host/gs_variant_check.cpp, which runs as a plain process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")


def test_gs_launch_variant(tmp_path):
    exe = tmp_path / "gs_variant_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "gs_variant_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all gs variant checks passed" in out.stdout
