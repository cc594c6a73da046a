"""plan_step (csrc/step_plan.hpp): which kernels a search step runs, as a
function of the batch, the options and what the caller wants.  Every path
gives the same verdicts, so these rules are pinned here, on the CPU, through
tests/step_plan_main.cpp (host C++ only, no HIP).  Expected values are
derived from the rules as they stood inside dev_search before they moved."""
import os
import shutil
import subprocess

import pytest

from lincheck import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not shutil.which(CXX), reason="no ROCm clang++")

IN_FIELDS = ("K n_events cu_count t0_only table taggable seg_pays validated has_events16 algorithm flags path_flags "
             "spec_segs max_configs want_peak want_final want_n_final res_host allow_async spec8_waves ws_words "
             "fin_words ws_max_bytes").split()
OUT_FIELDS = ("wgl_only competition t0_step async split spec segs exact ev16 t0_wide g0 strict gen_validate "
              "side_validate spec_vblocks spec_vfirst t0_path ev_word_bytes").split()
NONE, LATTICE, SPEC, SEGMENTS = N.LC_T0_PATH_NONE, N.LC_T0_PATH_LATTICE, N.LC_T0_PATH_SPEC, N.LC_T0_PATH_SEGMENTS
COUNT_PROBES = 1  # LC_OPT_COUNT_PROBES

# :linear on 256 CUs, a validated register-tier batch, verdicts only, no probe
# counting, budget 2^20, the 8-wave k_spec build, 3 * 16 * 64 workspace words
# (12,288 B) per key and segment, the 8 GiB cap
BASE = dict(K=1000, n_events=0, cu_count=256, t0_only=1, table=0, taggable=0, seg_pays=0, validated=1, has_events16=0,
            algorithm=N.LC_ALGO_LINEAR, flags=0, path_flags=0, spec_segs=0, max_configs=1 << 20, want_peak=0,
            want_final=0, want_n_final=0, res_host=0, allow_async=0, spec8_waves=8, ws_words=3 * 16 * 64,
            fin_words=2 * 64, ws_max_bytes=8 << 30)
FINALS = dict(want_final=1, want_n_final=1)
TAG = dict(taggable=1, seg_pays=1)
OFF = N.LC_PATH_SPLIT_OFF | N.LC_PATH_SPEC_OFF

# (what, StepIn fields that differ from BASE, StepPlan fields expected)
ROWS = [
    ("C2", dict(), dict(spec=1, segs=8, t0_wide=1, g0=1000, t0_path=SPEC, t0_step=1, split=0, exact=0, wgl_only=0)),
    ("K 1024", dict(K=1024), dict(spec=1, segs=8)),
    ("K 1025", dict(K=1025), dict(spec=1, segs=2)),
    ("K 2048", dict(K=2048), dict(t0_wide=1, g0=2048)),
    ("K 2049", dict(K=2049), dict(t0_wide=0, g0=2049)),
    ("C3 shard", dict(K=12500), dict(spec=1, segs=2, g0=4096, spec_vfirst=1, t0_path=SPEC)),
    ("one resident round", dict(K=512), dict(segs=8, spec_vfirst=0)),
    ("more than one resident round", dict(K=513), dict(segs=8, spec_vfirst=1)),
    ("workspace cap: fits", dict(K=349525), dict(spec=1, segs=2, t0_path=SPEC)),
    ("workspace cap: one key more", dict(K=349526), dict(spec=0, t0_path=LATTICE)),
    ("peaks wanted", dict(want_peak=1), dict(spec=0, t0_path=LATTICE)),
    ("finals, no peaks", FINALS, dict(spec=1, exact=1, segs=8, t0_path=SPEC)),
    ("finals, spec_segs 3", dict(FINALS, spec_segs=3), dict(spec=1, exact=1, segs=2)),
    ("finals, spec_segs 6", dict(FINALS, spec_segs=6), dict(spec=1, exact=1, segs=4)),
    ("finals, K 1025", dict(FINALS, K=1025), dict(spec=1, exact=1, segs=2)),
    ("spec_segs 6", dict(spec_segs=6), dict(spec=1, exact=0, segs=6)),
    ("budget below the register tier's", dict(max_configs=32767), dict(spec=0, split=0, t0_path=LATTICE)),
    ("quiescent points pay, K 64", dict(TAG, K=64), dict(split=1, spec=0, t0_path=SEGMENTS)),
    ("quiescent points pay, K 2049", dict(TAG, K=2049), dict(split=0, spec=1, segs=2, t0_path=SPEC)),
    ("SPLIT_ON", dict(K=2048, taggable=1, path_flags=N.LC_PATH_SPLIT_ON), dict(split=1, t0_path=SEGMENTS)),
    ("SPLIT_ON, not taggable", dict(K=64, path_flags=N.LC_PATH_SPLIT_ON), dict(split=0, spec=1, t0_path=SPEC)),
    ("SPLIT_OFF", dict(TAG, K=64, path_flags=N.LC_PATH_SPLIT_OFF), dict(split=0, spec=1, segs=8, t0_path=SPEC)),
    ("SPLIT_OFF | SPEC_OFF", dict(path_flags=OFF), dict(split=0, spec=0, t0_path=LATTICE)),
    ("COUNT_PROBES", dict(flags=COUNT_PROBES, allow_async=1), dict(t0_step=0, **{"async": 0}, spec=0, t0_path=LATTICE)),
    ("table model", dict(table=1, t0_only=0), dict(t0_step=0, t0_path=NONE, ev_word_bytes=0)),
    ("no keys", dict(K=0), dict(t0_step=0, spec=0, segs=0, g0=1, t0_path=NONE, ev_word_bytes=0, side_validate=0)),
    ("async to host memory", dict(allow_async=1, res_host=1), {"async": 0, "t0_step": 1}),
    ("async, competition", dict(allow_async=1, algorithm=N.LC_ALGO_COMPETITION), {"async": 0, "competition": 1}),
    ("async", dict(allow_async=1), {"async": 1, "competition": 0}),
    ("async not asked", dict(), {"async": 0}),
    ("unvalidated, spec, K 1000", dict(validated=0),
     dict(strict=1, spec=1, side_validate=0, gen_validate=0, spec_vblocks=256)),
    ("unvalidated, spec, K 100", dict(validated=0, K=100), dict(strict=1, spec=1, side_validate=0, spec_vblocks=100)),
    ("unvalidated, SPEC_OFF", dict(validated=0, path_flags=N.LC_PATH_SPEC_OFF),
     dict(strict=1, side_validate=1, gen_validate=0, spec_vblocks=0)),
    ("unvalidated, beyond the register tier", dict(validated=0, t0_only=0),
     dict(strict=0, gen_validate=1, side_validate=1, t0_step=0, t0_path=LATTICE)),
    ("validated", dict(), dict(strict=0, gen_validate=0, side_validate=0, spec_vblocks=0)),
    ("events16, spec", dict(has_events16=1), dict(spec=1, ev16=1, ev_word_bytes=2)),
    ("events16, lattice", dict(has_events16=1, path_flags=OFF), dict(spec=0, ev16=0, ev_word_bytes=4)),
    ("32-bit words, spec", dict(), dict(ev16=0, ev_word_bytes=4)),
    ("algorithm WGL", dict(algorithm=N.LC_ALGO_WGL), dict(wgl_only=1)),
]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_plan") / "step_plan_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "step_plan_main.cpp"), "-o", exe], check=True, timeout=120)
    text = "".join(" ".join(str(int(dict(BASE, **delta)[f])) for f in IN_FIELDS) + "\n" for _, delta, _ in ROWS)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(ROWS)
    return {what: dict(zip(OUT_FIELDS, map(int, line.split()))) for (what, _, _), line in zip(ROWS, lines)}


@pytest.mark.parametrize("what", [r[0] for r in ROWS])
def test_plan(plans, what):
    want = next(r[2] for r in ROWS if r[0] == what)
    got = {f: plans[what][f] for f in want}
    assert got == want, plans[what]


def test_header_is_host_only():
    """step_plan.hpp stays free of HIP: the rules compile (and are tested)
    with a plain host compiler."""
    src = open(os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc", "step_plan.hpp")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert includes == ["<algorithm>", "<cstdint>", '"../../include/lincheck.h"']
