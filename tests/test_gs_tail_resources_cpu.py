"""Build-time conditions of form 7's fused launch with its short remainder tile staged in LDS (spk_k_iter.hip
gs_fused_tail_kernel<NG, MP, AH>, SPK_GS_TAIL; mdot_tiles in spk_device.hpp): the launch waits inside the kernel for its
own workgroups, so the staging area and the epilogue must leave the floors of the launch without it untouched.  Checked on
the compiler's resource remark for gfx950, for every instantiation that can be launched -- the default launch's (keep set
and kGsAhead loads ahead of the wait) for NG = 1..5 and MP = 0, 4, 8: no scratch, no VGPR spill, <= 256 VGPR + AGPR, two
waves per SIMD, <= 160 KiB of LDS per workgroup; and the LDS arithmetic of kGsTailMax: the staging area is
kGsTailSrc x kGsTailMax double2 beside what the same launch without it takes.
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
LDS_CU = 160 * 1024
MAX_VALUES = 40   # GsArgs::cnt: the vectors and planes of one reduction


def _remarks(tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spk_k_iter.hip"), "-o", str(tmp_path / "iter.o")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    tail, plain = {}, {}
    for block in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        r = {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in FIELDS.items()}
        m = re.match(r"\S*gs_fused_tail_kernelILi(\d)ELi(\d)ELi(\d)EE", block)
        if m:
            key = tuple(int(g) for g in m.groups())
            assert key not in tail, key
            tail[key] = r
        m = re.match(r"\S*gs_fused_kernelILi(\d)ELi(\d)ELb1ELi(\d)EE", block)
        if m:
            plain[tuple(int(g) for g in m.groups())] = r
    return tail, plain


def _declared():
    """kGsAhead of spk_k_iter.hip as {(ng, mp): ah}; kGsTailMax and kGsTailSrc of spk_device.hpp."""
    with open(os.path.join(CSRC, "spk_k_iter.hip")) as fh:
        src = fh.read()
    m = re.search(r"constexpr int kGsAhead\[3\]\[5\] = \{(.*?)\};", src, re.S)
    rows = re.findall(r"\{([^{}]*)\}", m.group(1))
    ahead = {(ng, mp): int(v) for mp, row in zip((0, 4, 8), rows) for ng, v in enumerate(row.split(","), 1)}
    with open(os.path.join(CSRC, "spk_device.hpp")) as fh:
        m = re.search(r"constexpr int kGsTailMax = (\d+), kGsTailSrc = (\d+);", fh.read())
    return ahead, int(m.group(1)), int(m.group(2))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_instantiation_with_the_remainder_staged_keeps_the_floors(tmp_path):
    tail, plain = _remarks(tmp_path)
    ahead, r_max, n_src = _declared()
    assert n_src == MAX_VALUES + 1   # w~ beside them
    for key, r in sorted(tail.items()):
        print("gs_fused_tail_kernel<NG=%d, MP=%d, AH=%d>" % key, r)
    assert set(tail) == {(ng, mp, ah) for (ng, mp), ah in ahead.items()}, sorted(tail)
    area = n_src * r_max * 16   # double2
    for key, r in tail.items():
        assert r["scratch"] == 0 and r["vspill"] == 0, (key, r)
        assert r["vgpr"] + r["agpr"] <= 256 and r["waves"] == 2, (key, r)   # one 512-thread workgroup per CU
        assert r["lds"] <= LDS_CU, (key, r)
        # beside the keep set (four vector-tiles of 32 KiB) and the reduction buffers of the launch without it
        assert r["lds"] == plain[key]["lds"] + area and plain[key]["lds"] >= 4 * 32768, (key, r, plain[key])
    # kGsTailMax is the largest power of two whose area fits what the launch without it leaves free
    free = LDS_CU - max(r["lds"] for r in plain.values())
    assert area <= free < 2 * area, (area, free)
