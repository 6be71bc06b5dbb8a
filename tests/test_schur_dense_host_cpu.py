"""The host-pure step of the exact Schur complement (csrc/spk_host.cpp: schur_dense_factor -- symmetrise, Cholesky, the
pivot rule that refuses a rank-deficient B) against brute force, without a GPU and without ROCm: compiled with g++ and the
sanitizers together with one self-checking program (tests/host/schur_dense_check.cpp), which runs as a plain process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")


def test_schur_dense_factor(tmp_path):
    exe = tmp_path / "schur_dense_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(CSRC, "spk_host.cpp"), os.path.join(ROOT, "tests", "host", "schur_dense_check.cpp"),
                           "-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all dense Schur host checks passed" in out.stdout
