"""The counter kernels' resources, read from libcounter_kernels.so's code
object (no GPU): which kernels the library holds, that none of them has
scratch, and their VGPR and LDS figures as DESIGN.md section 3.14 records
them.  liblincheck.so links the library by its own directory and holds none of
its kernels."""
import os
import re
import subprocess

import pytest

from test_occupancy import LDS_PER_CU, LLVM, SO

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNEL_LIB = os.path.join(os.path.dirname(SO), "libcounter_kernels.so")
# stem -> its instantiations (items per thread), or None for a plain kernel
KERNELS = {"k_counter_tile": (1, 8), "k_counter_carry": None, "k_counter_apply": (1, 8), "k_counter_judge_tile": (1, 8),
           "k_counter_judge": (1, 8)}


def code_object_kernels(lib, tmp):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in {LLVM}")
    fat = str(tmp / "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib, str(tmp / "x")],
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
            if m:
                out[m.group(1)] = {k: int(v) for k, v in re.findall(
                    r"\.(vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", block)}
    return out


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return code_object_kernels(KERNEL_LIB, tmp_path_factory.mktemp("counter_kernels"))


def named(kernels, stem, ipt):
    """The kernel `stem` (its <ipt> instantiation) by its mangled name."""
    tag = f"{len(stem)}{stem}" + (f"ILi{ipt}E" if ipt else "E")
    hit = [n for n in kernels if tag in n]
    assert len(hit) == 1, (tag, sorted(kernels))
    return hit[0]


CASES = [(stem, ipt) for stem, ipts in KERNELS.items() for ipt in (ipts or (None,))]


def test_the_library_holds_exactly_the_counter_kernels(kernels):
    assert len(kernels) == len(CASES) == 9, sorted(kernels)
    assert len({named(kernels, s, i) for s, i in CASES}) == 9


@pytest.mark.parametrize("stem, ipt", CASES)
def test_kernel_resources(kernels, stem, ipt):
    """No scratch and no spills.  At most 128 VGPRs: a workgroup is four
    waves, one per SIMD, and at 128 a SIMD's 512 registers hold four waves, so
    a CU keeps four workgroups resident, each lane with its tile's loads (up
    to twelve 16-byte ones in k_counter_judge<8>) in flight -- what a kernel
    that only streams needs.  An eighth of the CU's LDS per workgroup, so LDS
    never limits that."""
    name = named(kernels, stem, ipt)
    k = kernels[name]
    print(stem, ipt, k)
    assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0, f"{name}: {k}"
    assert k["vgpr_count"] <= 128, f"{name}: {k}"
    assert 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, f"{name}: {k}"


def test_the_figures_design_records(kernels):
    """DESIGN.md 3.14's table is this build's."""
    text = open(os.path.join(os.path.dirname(__file__), "..", "DESIGN.md")).read()
    for stem, ipt in CASES:
        k = kernels[named(kernels, stem, ipt)]
        label = f"`{stem}<{ipt}>`" if ipt else f"`{stem}`"
        row = f"| {label} | {k['vgpr_count']} | {k['group_segment_fixed_size']} | 0 |"
        assert row in text, row


def test_liblincheck_links_it_and_holds_none_of_its_kernels(tmp_path):
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-d", SO], check=True, capture_output=True, text=True).stdout
    assert "libcounter_kernels.so" in out and "$ORIGIN" in out
    assert not [n for n in code_object_kernels(SO, tmp_path) if "k_counter" in n]
