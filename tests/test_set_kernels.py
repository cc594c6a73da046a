"""The set kernels' resources, read from the built library's gfx950 code
objects (no GPU needed): none keeps a private segment (no scratch), and
k_set_small's LDS lets six workgroups share a CU, as csrc/set_plan.hpp says.
The library's .hip_fatbin holds one offload bundle per source file; each is
unbundled and its kernel descriptors read (llvm-readelf --notes)."""
import os
import re
import subprocess

import pytest

from test_occupancy import LDS_PER_CU, LLVM, SO

NAMES = ["k_set_small", "k_set_mark", "k_set_classify", "k_set_scan"]
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in {LLVM}")
    tmp = tmp_path_factory.mktemp("set_kernels")
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
            if m and "k_set_" in m.group(1):
                out[m.group(1)] = {k: int(v) for k, v in re.findall(
                    r"\.(vgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", block)}
    return out


@pytest.mark.parametrize("stem", NAMES)
def test_no_scratch(kernels, stem):
    mine = {n: k for n, k in kernels.items() if stem in n}
    assert len(mine) == (1 if stem in ("k_set_mark", "k_set_scan") else 2), sorted(kernels)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, f"{name}: {k}"


def test_lds_tier_share(kernels):
    small = {n: k for n, k in kernels.items() if "k_set_small" in n}
    assert small
    for name, k in small.items():
        assert LDS_PER_CU // k["group_segment_fixed_size"] >= 6, f"{name}: {k}"
        assert k["vgpr_count"] <= 80, f"{name}: {k}"  # 6 workgroups x 4 waves = 6 waves per SIMD: 512 / 6 registers
