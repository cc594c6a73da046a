"""csrc/counter_plan.hpp on the CPU, through tests/counter_plan_main.cpp: tile
counts, the offset entries each tile marks its heads from, the head bytes
k_counter_tile records and the carry kernel's chunks, at the edges the GPU
tests run.  Expected values follow from the rules stated in that header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")
CXX = shutil.which("g++")

pytestmark = pytest.mark.skipif(not CXX, reason="no g++")
ANY, FIRST = 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("counter_plan") / "plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "counter_plan_main.cpp"), "-o", out], check=True, timeout=120)
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    return [[int(x) for x in line.split()] for line in r.stdout.strip().split("\n")]


def series(exe, tile, counts):
    rows = run(exe, f"series {tile} {len(counts)} " + " ".join(map(str, counts)) + "\n")
    (n, tiles, chunks), per, (last,) = rows[0], rows[1:-1], rows[-1]
    assert len(per) == tiles
    return dict(n=n, tiles=tiles, chunks=chunks, first=[p[0] for p in per] + [last], heads=[p[1] for p in per])


def test_tiles_the_kernels_are_built_for(exe):
    assert run(exe, "tile 0\ntile 256\ntile 2048\ntile 512\ntile 255\ntile 4096\n") == [[2048], [256], [2048], [0], [0], [0]]


@pytest.mark.parametrize("n, tiles", [(1, 1), (255, 1), (256, 1), (257, 2), (3 * 256 + 1, 4)])
def test_one_key_has_one_head_at_the_first_tile(exe, n, tiles):
    s = series(exe, 256, [n])
    assert (s["n"], s["tiles"], s["chunks"]) == (n, tiles, 1)
    assert s["heads"] == [ANY | FIRST] + [0] * (tiles - 1)  # the tiles after the first hold no head
    assert s["first"] == [0] + [1] * (tiles - 1) + [2]


@pytest.mark.parametrize("at", [255, 256, 257])
def test_a_key_boundary_around_a_tile_boundary(exe, at):
    s = series(exe, 256, [at, 300])
    # key 1 starts in tile 0 (at 255), at the start of tile 1 (256) or inside it (257)
    want = {255: [ANY | FIRST, 0, 0], 256: [ANY | FIRST, ANY | FIRST, 0], 257: [ANY | FIRST, ANY, 0]}[at]
    assert s["tiles"] == 3 and s["heads"] == want
    assert s["first"][0] == 0 and s["first"][-1] == 3
    assert s["first"][1] == (2 if at == 255 else 1)


def test_empty_keys_and_many_heads_in_one_tile(exe):
    # keys: 3, 0, 0, 2, 0 items -> heads at items 0 and 3; entries 1, 2 repeat item 3, entries 4, 5 equal n
    s = series(exe, 256, [3, 0, 0, 2, 0])
    assert s["n"] == 5 and s["tiles"] == 1 and s["heads"] == [ANY | FIRST] and s["first"] == [0, 6]
    # no items at all: no tiles, nothing to launch
    s = series(exe, 256, [0, 0])
    assert s["n"] == 0 and s["tiles"] == 0 and s["chunks"] == 0 and s["first"] == [3]
    s = series(exe, 256, [])
    assert s["tiles"] == 0 and s["first"] == [1]
    # 300 keys of one item: tile 0 takes entries 0..255, tile 1 the rest and the closing entry
    s = series(exe, 256, [1] * 300)
    assert s["first"] == [0, 256, 301] and s["heads"] == [ANY | FIRST, ANY | FIRST]


def test_the_carry_kernels_chunks(exe):
    assert series(exe, 256, [256 * 256])["chunks"] == 1
    s = series(exe, 256, [257 * 256 + 1])
    assert s["tiles"] == 258 and s["chunks"] == 2
    assert series(exe, 2048, [3 * 2048 + 1])["tiles"] == 4
    # a trailing key that ends exactly at a tile's end starts no tile of its own
    s = series(exe, 2048, [2048, 2048])
    assert s["tiles"] == 2 and s["heads"] == [ANY | FIRST, ANY | FIRST] and s["first"] == [0, 1, 3]
