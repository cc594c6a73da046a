"""Shared test helpers: run the device and the oracle on the same history;
read the built library's kernel metadata."""
import os
import re
import subprocess

import numpy as np
import pytest

import cref
from lincheck import history as H
from lincheck.checker import Device, Packed

CAUSE = {"none": 0, "nonlin": 1, "budget": 2, "window": 3, "states": 4}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "jepsen-etcd-demo_amd", "lincheck", "liblincheck.so")
LLVM = "/opt/rocm/llvm/bin"


def code_object_kernels(tmp_path):
    """Kernel metadata (llvm-readelf --notes) of every source file's gfx950
    code object: the library's .hip_fatbin section is one offload bundle per
    .hip file, back to back."""
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in {LLVM}")
    if not os.path.exists(SO):
        pytest.skip("liblincheck.so not built")
    fat = str(tmp_path / "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", SO, str(tmp_path / "x")],
                   check=True, capture_output=True)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)]
    out = {}
    for i, b in enumerate(starts):
        part, co = str(tmp_path / f"b{i}.bin"), str(tmp_path / f"k{i}.co")
        open(part, "wb").write(data[b:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for block in re.split(r"\n  - \.agpr_count:", notes):
            m = re.search(r"\.name:\s+(\S+)", block)
            if m:
                out[m.group(1)] = {k: int(v) for k, v in re.findall(
                    r"\.(vgpr_count|group_segment_fixed_size|private_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)",
                    block)}
    return out


def device_vs_oracle(hist: H.History, dev: Device, budget=None, check_peak=True, verdicts_only=False):
    """Assert bit-exact agreement of the device search with the C restatement.
    verdicts_only: the library's fast path (no sizes, configs or probes asked
    for) -- verdicts, causes and failing events must still be identical."""
    budget = budget or dev.budget
    packed = Packed(hist)
    res = dev.check(packed, verdicts_only=verdicts_only)
    if verdicts_only:
        check_peak = False
    keys, orc = cref.check_history(hist.as_c(), budget=budget, threads=8)
    assert list(keys) == packed.keys
    np.testing.assert_array_equal(res.valid, orc["valid"], err_msg="valid?")
    np.testing.assert_array_equal(res.cause, orc["cause"], err_msg="cause")
    np.testing.assert_array_equal(res.fail_event, orc["fail_event"], err_msg="fail event")
    done = orc["cause"] != CAUSE["budget"]
    if check_peak:
        np.testing.assert_array_equal(res.peak[done], orc["peak"][done], err_msg="peak configs")
    if done.all() and dev.count_probes and not verdicts_only:
        assert res.stats["probes"] == int(orc["probes"].sum())
    return packed, res, orc


# ---- counterexample shaping -----------------------------
def state_ids(packed: Packed, i: int) -> dict:
    """Model-state value -> packed state id for key i (ids may come from a
    table shared by every key, so walk it to its end)."""
    out = {}
    for s in range(1 << 16):
        try:
            out[packed.state_value(i, s)] = s
        except Exception:
            break
    return out


def oracle_state_value(st, model: str):
    """The restatement's state as the value lc_pack interns (mutex: locked -> 1)."""
    if model == "mutex":
        return 1 if st else None
    return st


def encode_finals(packed: Packed, i: int, a, model: str, limit: int = 10):
    """The restatement's final configs in the device's record layout
    (lo = slots 0..63, hi = slots 64..111 | state << 48)."""
    ids = state_ids(packed, i)
    out = np.zeros((limit, 2), np.uint64)
    n = 0
    for st, L in a.final_configs[:limit]:
        mask = 0
        for q in L:
            mask |= 1 << a.final_slots[q]
        out[n, 0] = mask & ((1 << 64) - 1)
        out[n, 1] = (mask >> 64) | (ids[oracle_state_value(st, model)] << 48)
        n += 1
    return out, n


def path_tuple(path, model: str):
    """A rendered :final-paths entry as the restatement's tuple form."""
    def state(m):
        if "msg" in m:
            return "inconsistent"
        v = m["locked?"] if model == "mutex" else m["value"]
        return v
    return tuple(((e["op"]["index"] if e["op"] is not None else None), state(e["model"])) for e in path)


def config_tuple(cfg, model: str):
    """A rendered :configs entry as (state, frozenset of linearized :index)."""
    m = cfg["model"]
    v = m["locked?"] if model == "mutex" else m["value"]
    return (v, frozenset(o["index"] for o in cfg["linearized"]))
