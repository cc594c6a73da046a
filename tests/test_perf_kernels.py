"""The perf kernels' resources, read from the built library's gfx950 code
objects (no GPU needed), the way tests/test_set_kernels.py reads the set
kernels': none keeps a private segment (no scratch), and k_perf_select_lds's
LDS lets the workgroups csrc/perf_plan.hpp promises share a CU."""
import os
import re
import subprocess

import pytest

from test_occupancy import LDS_PER_CU, LLVM, SO

NAMES = ["k_perf_count", "k_perf_scan", "k_perf_scatter", "k_perf_select_lds", "k_perf_hbm_init", "k_perf_hbm_hist",
         "k_perf_hbm_pick"]
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
LDS_SHARE = 5    # csrc/perf_plan.hpp: PERF_LDS_SHARE
LDS_MAX = 2048   # PERF_LDS_MAX points of 16 bytes


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in {LLVM}")
    tmp = tmp_path_factory.mktemp("perf_kernels")
    fat = str(tmp / "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", SO, str(tmp / "x")],
                   check=True, capture_output=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = {}
    for i, b in enumerate(starts):
        part, co = str(tmp / f"bundle{i}.bin"), str(tmp / f"k{i}.co")
        with open(part, "wb") as f:
            f.write(data[b:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for block in re.split(r"\n  - \.agpr_count:", notes):
            m = re.search(r"\.name:\s+(\S+)", block)
            if m and "k_perf_" in m.group(1):
                out[m.group(1)] = {k: int(v) for k, v in re.findall(
                    r"\.(vgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", block)}
    return out


@pytest.mark.parametrize("stem", NAMES)
def test_no_scratch(kernels, stem):
    mine = {n: k for n, k in kernels.items() if stem in n}
    assert len(mine) == 1, sorted(kernels)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, f"{name}: {k}"


def test_every_perf_kernel_is_listed(kernels):
    assert len(kernels) == len(NAMES), sorted(kernels)


def test_lds_tier_share(kernels):
    (name, k), = [(n, k) for n, k in kernels.items() if "k_perf_select_lds" in n]
    assert k["group_segment_fixed_size"] == LDS_MAX * 16, f"{name}: {k}"
    assert LDS_PER_CU // k["group_segment_fixed_size"] == LDS_SHARE, f"{name}: {k}"
    # 5 workgroups x 4 waves = 5 waves per SIMD: 512 / 5 registers each
    assert k["vgpr_count"] <= 512 // LDS_SHARE, f"{name}: {k}"


def test_streaming_kernels_leave_the_cu_to_its_waves(kernels):
    """The count and scatter tiles are a few KiB: LDS never limits occupancy
    (8 workgroups of 4 waves fill a CU's 32 wave slots)."""
    for stem in ("k_perf_count", "k_perf_scatter", "k_perf_hbm_hist"):
        (name, k), = [(n, k) for n, k in kernels.items() if stem in n]
        assert LDS_PER_CU // k["group_segment_fixed_size"] >= 8, f"{name}: {k}"
