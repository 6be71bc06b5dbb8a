"""Build-time conditions of form 7's fused launch (spk_k_iter.hip gs_fused_kernel, with and without its keep set): the
launch waits inside the kernel for its own workgroups, so all 256 of them (512 threads each) must be resident at once --
one per CU, two waves per SIMD -- and a kept operand must really stay on chip.  Checked on the compiler's resource remark
for gfx950, for every instantiation: no scratch, no VGPR spill, <= 256 VGPR + AGPR, <= 160 KiB of LDS per workgroup.
No GPU needed; skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

FIELDS = {"vgpr": r"VGPRs", "agpr": r"AGPRs", "scratch": r"ScratchSize \[bytes/lane\]", "waves": r"Occupancy \[waves/SIMD\]",
          "vspill": r"VGPRs Spill", "lds": r"LDS Size \[bytes/block\]"}


def _remarks(tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spk_k_iter.hip"), "-o", str(tmp_path / "iter.o")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        m = re.match(r"\S*gs_fused_kernelILi(\d)ELi(\d)ELb(\d)E", block)
        if m:
            out[tuple(int(g) for g in m.groups())] = {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in FIELDS.items()}
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_fused_instantiation_fits_one_workgroup_per_cu_without_scratch(tmp_path):
    res = _remarks(tmp_path)
    assert sorted(res) == sorted((ng, mp, keep) for ng in range(1, 6) for mp in (0, 4, 8) for keep in (0, 1))
    for key, r in sorted(res.items()):
        print("gs_fused_kernel<NG=%d, MP=%d, KEEP=%d>" % key, r)
    for key, r in res.items():
        assert r["scratch"] == 0 and r["vspill"] == 0, (key, r)
        assert r["vgpr"] + r["agpr"] <= 256 and r["waves"] >= 2, (key, r)
        assert r["lds"] <= 163840, (key, r)
        # the keep set is there: four vector-tiles of 32 KiB in LDS beside the reduction buffers
        assert (r["lds"] >= 4 * 32768) == bool(key[2]), (key, r)
