"""Build-time shape of the A-block product kernels and the FP32 sweeps on the same layouts (spk_k_spmv.hip, spk_k_dict.hip,
spk_k_dict3.hip), read from the compiler's resource remark for gfx950: the set of instantiations is the one the launchers
dispatch over (dispatch_product in spk_device.hpp: ACC x RIDE x BT without BT + RIDE), nothing spills, and no kernel holds
fewer waves per SIMD than it did before the kernels shared one frame.  Register counts are printed, not asserted.
No GPU needed; skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saddle_point_petsc_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

FIELDS = {"vgpr": r"VGPRs", "agpr": r"AGPRs", "sgpr": r"SGPRs", "scratch": r"ScratchSize \[bytes/lane\]",
          "waves": r"Occupancy \[waves/SIMD\]", "vspill": r"VGPRs Spill", "lds": r"LDS Size \[bytes/block\]"}
FILES = ("spk_k_spmv.hip", "spk_k_dict.hip", "spk_k_dict3.hip")
NAME = re.compile(r"_ZN3spk1k\d+((?:spmv|jacobi_sweep_f32)\w*?_kernel)(?:I((?:L[bi]\d+E)+)E)?")

PRODUCTS = {"spmv_stream_kernel": 2, "spmv_bcsr_kernel": 6, "spmv_bcsr3_kernel": 4, "spmv_dict_kernel": 30,
            "spmv_dict2_kernel": 12, "spmv_dict3_kernel": 18}
SWEEPS = {"jacobi_sweep_f32_dict_kernel": 5, "jacobi_sweep_f32_dict3_kernel": 3, "jacobi_sweep_f32_kernel": 1,
          "jacobi_sweep_f32_b2_kernel": 1, "jacobi_sweep_f32_b3_kernel": 1}
STATIC_LDS = {"spmv_stream_kernel": 16480, "spmv_bcsr_kernel": 16448, "spmv_bcsr3_kernel": 18528}


def _floor(name, a):
    """Waves per SIMD of the kernels before they shared one frame (a: the template arguments in order)."""
    if name == "spmv_dict_kernel":  # <BS, ACC, RIDE, BT, U3>
        bs, acc, _, bt, _ = a
        if bs == 2:
            return 4 if not acc and not bt else 3
        return 2 if bt else 3
    if name == "spmv_dict2_kernel":  # <ACC, RIDE, BT, KM, UNI>
        acc, _, _, _, uni = a
        return (2 if acc else 3) if uni else 2
    if name in ("spmv_dict3_kernel", "jacobi_sweep_f32_dict3_kernel"):
        return 2
    if name == "jacobi_sweep_f32_dict_kernel":  # <BS, U3>
        return 4 if a[0] == 2 else 7
    return 8  # stream, bcsr, bcsr3 and the three sweeps beside them


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("product_resources")
    out = {}
    for f in FILES:
        cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-I/opt/rocm/include",
               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, f), "-o", str(tmp / (f + ".o"))]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        assert p.returncode == 0, p.stderr[-2000:]
        for block in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
            m = NAME.match(block)
            if m:
                args = tuple(int(v) for v in re.findall(r"L[bi](\d+)E", m.group(2) or ""))
                out[(m.group(1), args)] = {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in FIELDS.items()}
    for (name, args), r in sorted(out.items()):
        print("%-30s %-22s vgpr %3d agpr %3d sgpr %3d waves %d lds %5d scratch %d" % (
            name, "<" + ",".join(map(str, args)) + ">", r["vgpr"], r["agpr"], r["sgpr"], r["waves"], r["lds"], r["scratch"]))
    return out


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_the_instantiations_are_those_the_launchers_dispatch_over(remarks):
    count = Counter(name for name, _ in remarks)
    assert {k: count[k] for k in PRODUCTS} == PRODUCTS and sum(PRODUCTS.values()) == 72
    assert {k: count[k] for k in SWEEPS} == SWEEPS and sum(SWEEPS.values()) == 11
    assert set(count) == set(PRODUCTS) | set(SWEEPS), sorted(count)


@needs_hipcc
def test_no_scratch_no_spill_and_no_occupancy_lost(remarks):
    for (name, args), r in sorted(remarks.items()):
        assert r["scratch"] == 0 and r["vspill"] == 0, (name, args, r)
        assert r["waves"] >= _floor(name, args), (name, args, r, _floor(name, args))


@needs_hipcc
def test_static_lds_of_the_tiled_products(remarks):
    for (name, args), r in sorted(remarks.items()):
        if name in STATIC_LDS:
            assert r["lds"] == STATIC_LDS[name], (name, args, r)
