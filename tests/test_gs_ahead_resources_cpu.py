"""Build-time conditions of form 7's fused launch with its loads ahead of the totals wait (spk_k_iter.hip
gs_fused_kernel<NG, MP, KEEP, AH>, SPK_GS_AHEAD): the second buffer of basis loads lives across the wait in registers the
tile loop would otherwise leave empty, so an instantiation holds as many vectors of it as fit without scratch -- kGsAhead
in spk_k_iter.hip says how many.  Checked on the compiler's resource remark for gfx950, for every instantiation the
build contains: no scratch, no VGPR spill, <= 256 VGPR + AGPR, two waves per SIMD, <= 160 KiB of LDS per workgroup, and
the AH built are the ones the table declares (no groups left to the L2: that constant was taken out).
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
        m = re.match(r"\S*gs_fused_kernelILi(\d)ELi(\d)ELb(\d)ELi(\d)EE", block)
        if m:
            key = tuple(int(g) for g in m.groups())
            assert key not in out, key
            out[key] = {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in FIELDS.items()}
    return out


def _declared():
    """kGsAhead as spk_k_iter.hip declares it: {(ng, mp): vectors requested ahead of the wait beyond the first group}."""
    with open(os.path.join(CSRC, "spk_k_iter.hip")) as fh:
        src = fh.read()
    m = re.search(r"constexpr int kGsAhead\[3\]\[5\] = \{(.*?)\};", src, re.S)
    rows = re.findall(r"\{([^{}]*)\}", m.group(1))
    assert len(rows) == 3
    ahead = {}
    for mp, row in zip((0, 4, 8), rows):
        vals = [int(v) for v in row.split(",")]
        assert len(vals) == 5
        for ng, v in enumerate(vals, 1):
            ahead[(ng, mp)] = v
    assert "KL2" not in src
    return ahead


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_fused_instantiation_with_loads_ahead_fits_and_is_the_declared_one(tmp_path):
    res = _remarks(tmp_path)
    ahead = _declared()
    assert all(0 <= v <= 4 for v in ahead.values())   # kGsG = 4: the tile loop's buffer is one group
    want = set()
    for (ng, mp), ah in ahead.items():
        want |= {(ng, mp, 0, 0), (ng, mp, 1, 0), (ng, mp, 1, ah)}   # no keep set; SPK_GS_AHEAD=0; the default
    for key, r in sorted(res.items()):
        print("gs_fused_kernel<NG=%d, MP=%d, KEEP=%d, AH=%d>" % key, r)
    assert set(res) == want, sorted(set(res) ^ want)
    for key, r in res.items():
        assert r["scratch"] == 0 and r["vspill"] == 0, (key, r)
        assert r["vgpr"] + r["agpr"] <= 256 and r["waves"] >= 2, (key, r)   # one 512-thread workgroup per CU
        assert r["lds"] <= 163840, (key, r)
        if key[2]:
            assert r["waves"] == 2 and r["lds"] >= 4 * 32768, (key, r)     # (the keep set's LDS allows no second one)
