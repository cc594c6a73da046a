"""The streaming set-full's host side without a GPU, beyond the packer
(tests/test_setfull_stream_pack.py):
  * the capacity and pass rules of csrc/setfull_stream_plan.hpp through
    tests/setfull_stream_plan_main.cpp; expected values follow from the rules
    stated in that header;
  * the packer under AddressSanitizer and UBSan: a stand-alone program
    (tests/setfull_stream_asan_main.cpp) built together with the one host
    source it needs, nothing preloaded, nothing loaded into Python;
  * the new kernels' resources, read from libsetfull_stream_kernels.so's code
    object."""
import os
import re
import shutil
import subprocess

import pytest

from test_occupancy import LDS_PER_CU, LLVM, SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = "/opt/rocm/llvm/bin/clang++"

needs_cxx = pytest.mark.skipif(not shutil.which(CXX), reason="no ROCm clang++")


# ---- plan ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("setfull_stream_plan") / "plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "setfull_stream_plan_main.cpp"), "-o", out], check=True, timeout=120)
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    return [list(map(int, line.split())) for line in r.stdout.strip().splitlines()]


def chunk(exe, keys, cap):
    lines = run(exe, f"chunk {len(keys)} {cap}\n" + "".join("%d %d %d\n" % k for k in keys))
    head = dict(zip("passes segs marks folds max_words total_words".split(), lines[0]))
    passes = [dict(zip("mark0 mark1 fold0 fold1 words".split(), l)) for l in lines[1:1 + head["passes"]]]
    return head, passes, [tuple(l) for l in lines[1 + head["passes"]:]]


@needs_cxx
def test_capacity_grows_in_blocks_of_256_ids_and_by_doubling(exe):
    assert [run(exe, f"blocks {n}\n")[0][0] for n in (0, 1, 255, 256, 257, 512, 513, 600)] == [0, 1, 1, 1, 2, 2, 3, 3]
    grow = lambda have, need: run(exe, f"grow {have} {need}\n")[0][0]  # noqa: E731
    assert grow(0, 0) == 64 and grow(0, 1) == 64 and grow(0, 64) == 64 and grow(0, 65) == 128
    assert grow(64, 65) == 128 and grow(64, 129) == 256 and grow(128, 100) == 128 and grow(128, 1000) == 1024


@needs_cxx
def test_row_passes_under_a_cap(exe):
    """600 ids are 3 blocks = 12 words per row; 40 rows are 480 words = 3,840 bytes."""
    key = [(600, 40, 10)]
    for cap in (0, 3840, 1 << 20):
        head, passes, segs = chunk(exe, key, cap)
        assert head == dict(passes=1, segs=1, marks=40, folds=3, max_words=480, total_words=480), cap
        assert segs == [(0, 40, 12, 0, 0)]
    head, passes, segs = chunk(exe, key, 3832)  # one word less: 39 whole rows, then the last one
    assert head == dict(passes=2, segs=2, marks=40, folds=6, max_words=468, total_words=480)
    assert segs == [(0, 39, 12, 0, 0), (0, 1, 12, 39, 0)]
    assert passes == [dict(mark0=0, mark1=39, fold0=0, fold1=3, words=468), dict(mark0=39, mark1=40, fold0=3, fold1=6, words=12)]
    head, passes, segs = chunk(exe, key, 15 * 12 * 8)  # 15 rows a pass: 15, 15, 10
    assert [s[1] for s in segs] == [15, 15, 10] and [s[3] for s in segs] == [0, 15, 30] and head["passes"] == 3
    head, passes, segs = chunk(exe, key, 8)  # a row is wider than the cap: one row per pass, above it
    assert head["passes"] == 40 and head["max_words"] == 12 and all(s[1] == 1 for s in segs)


@needs_cxx
def test_keys_share_passes_and_edge_keys(exe):
    keys = [(65, 2, 3),    # 1 block: 4 words x 2 rows
            (0, 3, 0),     # no ids (empty reads only): no matrix, no fold workgroup
            (500, 0, 0),   # adds only: a segment of no rows, its 2 blocks folded all the same
            (300, 5, 4)]   # 2 blocks: 8 words x 5 rows
    head, passes, segs = chunk(exe, keys, 1 << 20)
    assert head["passes"] == 1 and passes[0]["words"] == 8 + 40
    assert segs == [(0, 2, 4, 0, 0), (1, 3, 0, 2, 8), (2, 0, 8, 5, 8), (3, 5, 8, 5, 8)]
    assert head["marks"] == 2 + 5 and head["folds"] == 1 + 0 + 2 + 2
    # under a cap of 24 words: key 0 (8 words), then key 3's 5 rows as 2 + 3
    head, passes, segs = chunk(exe, keys, 24 * 8)
    assert [(s[0], s[1], s[3]) for s in segs] == [(0, 2, 0), (1, 3, 2), (2, 0, 5), (3, 2, 5), (3, 3, 7)]
    assert [p["words"] for p in passes] == [24, 24]
    # a row of 1,025 elements from element 0 is two mark workgroups, of 1,024 one
    assert chunk(exe, [(100, 1, 1025)], 1 << 20)[0]["marks"] == 2 and chunk(exe, [(100, 1, 1024)], 1 << 20)[0]["marks"] == 1


# ---- the packer under the sanitizers ----------------------------------------------------

@needs_cxx
def test_packer_runs_clean_under_asan_and_ubsan(tmp_path):
    out = str(tmp_path / "asan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "setfull_stream_asan_main.cpp"), os.path.join(CSRC, "host_setfull_stream.cpp"),
                    "-o", out], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-3000:]


# ---- the new kernels' resources (from the code object, no GPU) ---------------------------

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNEL_LIB = os.path.join(os.path.dirname(SO), "libsetfull_stream_kernels.so")
STEMS = ["k_sfs_reset", "k_sfs_mark", "k_sfs_fold", "k_sfs_finish"]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """The kernel descriptors of the library (as tests/test_setfull_host.py reads libsetfull_kernels.so's)."""
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in {LLVM}")
    tmp = tmp_path_factory.mktemp("setfull_stream_kernels")
    fat = str(tmp / "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", KERNEL_LIB, str(tmp / "x")],
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
                    r"\.(vgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", block)}
    return out


@pytest.mark.parametrize("stem", STEMS)
def test_kernel_resources(kernels, stem):
    """No scratch, at most 64 VGPRs (8 waves per SIMD) and an eighth of the
    CU's LDS per workgroup: DESIGN 3.12's occupancy target."""
    mine = {n: k for n, k in kernels.items() if stem in n}
    assert len(mine) == 1 and len(kernels) == len(STEMS), sorted(kernels)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, f"{name}: {k}"
        assert k["vgpr_count"] <= 64, f"{name}: {k}"
        assert 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, f"{name}: {k}"
        print(name, k)


def test_the_library_is_linked_by_its_own_directory():
    """liblincheck.so needs libsetfull_stream_kernels.so and finds it beside itself."""
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-d", SO], check=True, capture_output=True, text=True).stdout
    assert "libsetfull_stream_kernels.so" in out and "$ORIGIN" in out
