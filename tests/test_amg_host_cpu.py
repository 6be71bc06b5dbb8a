"""The host multigrid hierarchy (csrc/spk_amg_host.cpp over spk_amg_levels.hpp: the CSR algebra, Lanczos, the aggregation,
the grid prolongator, the coarse inverse, the two level loops, the rules on the options, the smoother's coefficients)
without a GPU and without ROCm: the host-pure sources are compiled with g++ and the sanitizers together with one
self-checking program (tests/host/amg_host_check.cpp), which goes through the C entry points Python uses and runs as a
plain process."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")


def test_amg_host_hierarchy(tmp_path):
    exe = tmp_path / "amg_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(CSRC, "spk_host.cpp"), os.path.join(CSRC, "spk_galerkin_host.cpp"),
                           os.path.join(CSRC, "spk_amg_host.cpp"), os.path.join(ROOT, "tests", "host", "amg_host_check.cpp"),
                           "-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all multigrid host checks passed" in out.stdout


def test_amg_host_unit_includes_nothing_from_rocm():
    """spk_amg_host.cpp, spk_amg_levels.hpp and spk_amg.hpp: standard headers, include/spk.h and the project's host-pure
    headers only (the compile above has no ROCm include path; this names the rule)."""
    own = {"spk.h", "spk_host.hpp", "spk_amg.hpp", "spk_amg_levels.hpp", "spk_galerkin_core.hpp", "spk_lanczos_core.hpp"}
    for name in ("spk_amg_host.cpp", "spk_amg_levels.hpp", "spk_amg.hpp"):
        src = open(os.path.join(CSRC, name)).read()
        incs = re.findall(r"^\s*#\s*include\s*(\S+)", src, re.M)
        assert incs, name
        for i in incs:
            std = re.fullmatch(r"<[a-z_]+>", i) is not None   # <vector>, <cstdint>: no directory, no .h
            assert std or (i.startswith('"') and os.path.basename(i.strip('"')) in own), (name, i)
