"""csrc/rows_plan.hpp and csrc/counter_pack_plan.hpp on the CPU, through
tests/counter_pack_plan_main.cpp: table slots, sort bits, block and tile
counts at 0, 1 and 2^k +- 1 rows and at the largest n, the error word and the
split sum.  Expected values follow from the rules stated in those headers."""
import os
import shutil
import subprocess

import pytest

import counter_pack_helpers as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(not CXX, reason="no g++")
MAX_ROWS = (1 << 31) - 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("counter_pack_plan") / "plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "counter_pack_plan_main.cpp"), "-o", out], check=True, timeout=120)
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    return r.stdout.strip().split("\n")


def ints(exe, text):
    return [[int(x) for x in line.split()] for line in run(exe, text)]


def pow2_at_least(x):
    p = 1
    while p < x:
        p <<= 1
    return p


SIZES = sorted({0, 1, MAX_ROWS} | {(1 << k) + d for k in (1, 8, 11, 16, 21, 30) for d in (-1, 0, 1)})


def test_constants(exe):
    assert ints(exe, "consts\n") == [[256, 8, 2048, MAX_ROWS, 16, 0xFFFFFFFF, 8]]


def test_slots_blocks_and_tiles(exe):
    got = ints(exe, "".join(f"rows {n}\n" for n in SIZES))
    for n, (slots, blocks, tiles, slot_blocks) in zip(SIZES, got):
        assert slots == max(256, pow2_at_least(2 * n)), n         # a power of two, load factor at most 1/2
        assert slots & (slots - 1) == 0 and slots >= 2 * n
        assert blocks == -(-n // 256) and tiles == -(-n // 2048) and slot_blocks == slots // 256
        assert slot_blocks < 1 << 31 and blocks < 1 << 31           # one launch's workgroups
    assert ints(exe, f"rows {MAX_ROWS + 1}\n")[0][0] == 0           # past the largest n: no table


def test_sort_bits(exe):
    maxes = [0, 1, 2, 3, 255, 256, 257, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    got = [b for (b,) in ints(exe, "".join(f"bits {m}\n" for m in maxes))]
    assert got == [max(1, m.bit_length()) for m in maxes]
    # the two sorts' keys are 32-bit: the bits of the key index and of the process index at any n
    for n, (kb, pb, limit) in zip(SIZES, ints(exe, "".join(f"sort {n}\n" for n in SIZES))):
        assert limit == 32 and kb <= limit and pb <= limit and kb + pb <= 64, n
        assert kb == max(1, n.bit_length()) and pb == max(1, max(n - 1, 0).bit_length())


def test_the_hash_is_the_one_the_tests_restate(exe):
    def murmur(k):
        k ^= k >> 33
        k = k * 0xff51afd7ed558ccd & ((1 << 64) - 1)
        k ^= k >> 33
        k = k * 0xc4ceb9fe1a85ec53 & ((1 << 64) - 1)
        return k ^ (k >> 33)
    keys = [0, 1, 2, 255, 256, 1 << 32, (1 << 63) - 1, (1 << 63) + 1, (1 << 64) - 1]
    assert [h for (h,) in ints(exe, "".join(f"hash {k}\n" for k in keys))] == [murmur(k) for k in keys]
    # multiples of a table's slot count spread over it
    assert len({murmur(512 * i) & 511 for i in range(512)}) > 256


def test_error_words_order_by_row_then_code(exe):
    rows = [0, 1, 7, MAX_ROWS - 1]
    words = {}
    for r in rows:
        for code in range(1, 8):
            (w, back_row, back_code, below), = ints(exe, f"word {r} {code}\n")
            assert (back_row, back_code, below) == (r, code, 1)
            words[(r, code)] = w
    assert sorted(words, key=words.get) == sorted(words)


def test_the_split_sum_passes_int64_exactly_past_its_maximum(exe):
    # (value, how many of it) lists; the last a batch of the largest n
    cases = [[(PH.I64_MAX, 1)], [(PH.I64_MAX, 1), (1, 1)], [(PH.I64_MAX - 1, 1), (1, 1)], [(1 << 62, 2)], [((1 << 62) - 1, 1), (1 << 62, 1)],
             [(0xFFFFFFFF, 5)], [(0xFFFFFFFF, MAX_ROWS)], [(PH.I64_MAX, 3)], [(0, 1)], [((1 << 32) - 1, 1 << 31), ((1 << 31) - 1, 1)],
             [((1 << 32) - 1, 1 << 31), (1 << 31, 1)]]
    text, want = "", []
    for values in cases:
        lo, hi = sum((v & 0xFFFFFFFF) * c for v, c in values), sum((v >> 32) * c for v, c in values)
        assert lo < 1 << 64 and hi < 1 << 64
        text += f"sum {lo} {hi}\n"
        want.append(int(sum(v * c for v, c in values) > PH.I64_MAX))
    assert want == [0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1]
    assert [x for (x,) in ints(exe, text)] == want


def test_the_messages(exe):
    got = run(exe, "".join(f"text {c}\n" for c in range(9)))
    assert got == ["-"] + list(PH.MESSAGES) + ["-"]
