"""Static checks on kernel source shapes that once hung a wave on the GPU.

Round 3: a `for (;;) ... break` walk loop in k_spec (device_spec.hip) was
compiled into an exec-masked loop whose exit hung the wave after its first
walk; it was replaced by fixed trip counts over uni()-uniform values.  The
kernel's LDS-flag waits (spec_wait, spec_ck_event) are loops of the same kind.
No run-time test can see a future edit that undoes that (the hang only
shows on the GPU), so the loop shapes are checked here, in the source."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jepsen-etcd-demo_amd", "csrc")


def _body(src: str, head: str) -> str:
    """The brace-balanced body of the first definition starting with head."""
    i = src.index(head)
    j = src.index("{", i)
    depth = 0
    for k in range(j, len(src)):
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[j:k + 1]
    raise AssertionError(f"unbalanced {head}")


def _code(text: str) -> str:
    """text without // comments"""
    return "\n".join(line.split("//")[0] for line in text.splitlines())


OPEN_LOOP = r"for\s*\(\s*;\s*;\s*\)|while\s*\(\s*(true|1)\s*\)"


def test_spec_walks_and_flag_waits_keep_fixed_trip_counts():
    src = _code(open(os.path.join(CSRC, "device_spec.hip")).read())
    head = re.search(r"__global__ __launch_bounds__\([^{;]*\) void k_spec\(", src)
    assert head, "k_spec's definition not found"
    k_spec = _body(src, head.group(0))
    bodies = {"k_spec": k_spec}
    for name, ret in (("spec_walk", "int"), ("spec_wait", "bool"), ("spec_ck_event", "int32_t")):
        bodies[name] = _body(src, f"__device__ __forceinline__ {ret} {name}(")
    for name, body in bodies.items():
        assert not re.search(OPEN_LOOP, body), f"an open loop in {name}"

    # the LDS-flag waits: a fixed trip count, every flag read a spec_load
    for name, flags in (("spec_wait", ("f",)), ("spec_ck_event", ("ck_e", "top_done"))):
        body = bodies[name]
        assert len(re.findall(r"\b(for|while|do)\b", body)) == 1, f"{name} has more than its one wait loop"
        at = re.search(r"for \(uint32_t it = 0; it < SPEC_WAIT_MAX; \+\+it\) ", body)
        assert at, f"{name}'s wait lost its fixed trip count"
        loop = _body(body[at.start():], at.group(0))
        rest, n_loads = re.subn(r"\bspec_load\([^()]*\)", "", loop)
        assert n_loads >= 1, f"{name} polls no flag"
        assert "__hip_atomic_load" not in rest
        for flag in flags:
            assert not re.search(r"\b%s\b" % flag, rest), f"{name} reads {flag} without spec_load"
    load = _body(src, "__device__ __forceinline__ int32_t spec_load(")
    assert re.search(r"\{\s*return uni\(__hip_atomic_load\(f, __ATOMIC_ACQUIRE, [^;]*\)\);\s*\}$", load), \
        "spec_load is no longer a uni() of an acquire load"

    # k_spec's walks: the wave's segment index and the scan for the next kept
    # segment branch on wave-uniform values only
    assert re.search(r"\bwv = uni\(\(uint32_t\)threadIdx\.x >> 6\)", k_spec), "the wave index is not made uniform"
    at = k_spec.index("const uint32_t s = wv;")
    start = k_spec.rindex("if (!plain) {", 0, at)
    assert not k_spec[start + len("if (!plain) {"):at].strip(), "the walks' block does not start at its segment index"
    walks = _body(k_spec[start:], "if (!plain) ")
    assert "const bool kept = s < eff && uni(s_cut[s]) >= 0;" in walks
    assert "while (v < eff && uni(s_cut[v]) < 0) ++v;" in walks
    uses = [m.start() for m in re.finditer(r"s_cut\[", walks)]
    assert len(uses) >= 2
    for u in uses:
        assert walks[:u].endswith("uni("), "s_cut read without uni(): " + walks[u:u + 40]


def test_wgl_work_loop_is_bounded():
    src = _code(open(os.path.join(CSRC, "device_wgl.hip")).read())
    body = _body(src, "__global__ __launch_bounds__(64) void k_wgl(")
    assert not re.search(r"for\s*\(\s*;\s*;\s*\)|while\s*\(\s*(true|1)\s*\)", body)
    assert re.search(r"for \(int32_t guard = 0; guard <= n_work; \+\+guard\)", body)
    assert "w = (int32_t)uni((uint32_t)w);" in body
    key = _body(src, "__device__ bool wgl_key(")
    assert re.search(r"for \(uint64_t it = 0; it < max_it; \+\+it\)", key), "the walk lost its step bound"
