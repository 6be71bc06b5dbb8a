"""Build-time conditions of form 7's fused launch (spk_k_iter.hip gs_fused_kernel<NG, MP, KEEP, AH> and
gs_fused_tail_kernel<NG, MP, AH>; the variants of spk_gs_launch.hpp).  The launch waits inside the kernel for its own
workgroups, so all 256 of them (512 threads each) must be resident at once -- one per CU, two waves per SIMD -- and what
a variant keeps on chip must really stay there: the keep set's four vector-tiles of 32 KiB in LDS; the loads ahead of the
totals wait in registers the tile loop would otherwise leave empty, as many vectors as fit without scratch (kGsAhead; no
groups left to the L2: that constant was taken out); the staged remainder's kGsTailSrc x kGsTailMax double2 of
LDS beside what the same launch without it takes.  Checked on the compiler's resource remark for gfx950, one compile, for
every instantiation the build contains -- exactly the ones kGsAhead declares: no scratch, no VGPR spill, <= 256 VGPR +
AGPR, <= 160 KiB of LDS per workgroup.  No GPU needed; skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

FIELDS = {"vgpr": r"VGPRs", "agpr": r"AGPRs", "scratch": r"ScratchSize \[bytes/lane\]", "waves": r"Occupancy \[waves/SIMD\]",
          "vspill": r"VGPRs Spill", "lds": r"LDS Size \[bytes/block\]"}
LDS_CU = 160 * 1024
MAX_VALUES = 40   # GsArgs::cnt: the vectors and planes of one reduction


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """{(ng, mp, keep, ah): resources} of gs_fused_kernel, {(ng, mp, ah): resources} of gs_fused_tail_kernel."""
    obj = tmp_path_factory.mktemp("gs_resources") / "iter.o"
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "spk_k_iter.hip"), "-o", str(obj)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    fused, tail = {}, {}
    for block in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        for pat, out in ((r"\S*gs_fused_kernelILi(\d)ELi(\d)ELb(\d)ELi(\d)EE", fused),
                         (r"\S*gs_fused_tail_kernelILi(\d)ELi(\d)ELi(\d)EE", tail)):
            m = re.match(pat, block)
            if m:
                key = tuple(int(g) for g in m.groups())
                assert key not in out, key
                out[key] = {k: int(re.search(f + r": (\d+)", block).group(1)) for k, f in FIELDS.items()}
    for key, r in sorted(fused.items()):
        print("gs_fused_kernel<NG=%d, MP=%d, KEEP=%d, AH=%d>" % key, r)
    for key, r in sorted(tail.items()):
        print("gs_fused_tail_kernel<NG=%d, MP=%d, AH=%d>" % key, r)
    print(len(fused) + len(tail), "instantiations")
    return fused, tail


@pytest.fixture(scope="module")
def declared():
    """kGsAhead of spk_gs_launch.hpp as {(ng, mp): ah}, its kGsTailMax and kGsTailSrc."""
    with open(os.path.join(CSRC, "spk_gs_launch.hpp")) as fh:
        src = fh.read()
    rows = re.findall(r"\{([^{}]*)\}", re.search(r"constexpr int kGsAhead\[3\]\[5\] = \{(.*?)\};", src, re.S).group(1))
    assert len(rows) == 3
    ahead = {}
    for mp, row in zip((0, 4, 8), rows):
        vals = [int(v) for v in row.split(",")]
        assert len(vals) == 5
        ahead.update({(ng, mp): v for ng, v in enumerate(vals, 1)})
    m = re.search(r"constexpr int kGsTailMax = (\d+), kGsTailSrc = (\d+);", src)
    assert "KL2" not in src + open(os.path.join(CSRC, "spk_k_iter.hip")).read()
    return ahead, int(m.group(1)), int(m.group(2))


def test_the_build_holds_exactly_the_declared_instantiations(remarks, declared):
    fused, tail = remarks
    ahead = declared[0]
    assert sorted(ahead) == [(ng, mp) for ng in range(1, 6) for mp in (0, 4, 8)]
    assert all(0 <= v <= 4 for v in ahead.values())   # kGsG = 4: the tile loop's buffer is one group
    want = set()
    for (ng, mp), ah in ahead.items():
        want |= {(ng, mp, 0, 0), (ng, mp, 1, 0), (ng, mp, 1, ah)}   # no keep set; SPK_GS_AHEAD=0; the default
    assert set(fused) == want and len(fused) == 45, sorted(set(fused) ^ want)
    assert set(tail) == {(ng, mp, ah) for (ng, mp), ah in ahead.items()} and len(tail) == 15, sorted(tail)


def test_every_fused_instantiation_fits_one_workgroup_per_cu_without_scratch(remarks):
    fused, _ = remarks
    for key, r in fused.items():
        assert r["scratch"] == 0 and r["vspill"] == 0, (key, r)
        assert r["vgpr"] + r["agpr"] <= 256 and r["waves"] >= 2, (key, r)   # one 512-thread workgroup per CU
        assert r["lds"] <= LDS_CU, (key, r)
        # the keep set is there: four vector-tiles of 32 KiB in LDS beside the reduction buffers
        assert (r["lds"] >= 4 * 32768) == bool(key[2]), (key, r)
        if key[2]:
            assert r["waves"] == 2, (key, r)     # (the keep set's LDS allows no second one)


def test_every_instantiation_with_the_remainder_staged_keeps_the_floors(remarks, declared):
    fused, tail = remarks
    _, r_max, n_src = declared
    assert n_src == MAX_VALUES + 1   # w~ beside them
    plain = {(ng, mp, ah): r for (ng, mp, keep, ah), r in fused.items() if keep}   # the launch without it
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
