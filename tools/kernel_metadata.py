#!/usr/bin/env python3
"""llvm-readelf --notes metadata of every gfx950 kernel in two builds of
liblincheck.so, side by side, as profiles/stream_exact_metadata.json and
profiles/stream_exact_set_metadata.json record it:

    tools/kernel_metadata.py PARENT.so HEAD.so OUT.json

VGPRs, SGPRs, LDS bytes, private segment bytes, VGPR and SGPR spill counts per
kernel; the parent's kernels that differ in the head, and the head's new ones;
and, per translation unit (named by its kernels), the SHA-256 of the code
object's .text section on both sides: equal hashes mean the unit's device code
is byte for byte the parent's."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
FIELDS = {"vgpr_count": "vgpr", "sgpr_count": "sgpr", "group_segment_fixed_size": "lds",
          "private_segment_fixed_size": "private", "vgpr_spill_count": "vgpr_spill", "sgpr_spill_count": "sgpr_spill"}


def kernels(so):
    """({kernel: metadata}, {the unit's kernel names joined: sha256 of its .text})"""
    out, text = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", so, os.path.join(tmp, "x")],
                       check=True, capture_output=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
        for i, b in enumerate(starts):
            part, co = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"k{i}.co")
            open(part, "wb").write(data[b:starts[i + 1] if i + 1 < len(starts) else len(data)])
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            names = []
            for block in re.split(r"\n  - \.agpr_count:", notes):
                m = re.search(r"\.name:\s+(\S+)", block)
                if m:
                    vals = dict(re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), block))
                    out[m.group(1)] = {short: int(vals.get(name, 0)) for name, short in FIELDS.items()}
                    names.append(m.group(1))
            if names:
                txt = os.path.join(tmp, f"t{i}.bin")
                subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.text={txt}", co, os.path.join(tmp, "y")],
                               check=True, capture_output=True)
                text[" ".join(sorted(names))] = hashlib.sha256(open(txt, "rb").read()).hexdigest()
    return out, text


def main(parent_so, head_so, out_json):
    (parent, ptext), (head, htext) = kernels(parent_so), kernels(head_so)
    doc = {
        "what": "llvm-readelf --notes metadata of every gfx950 kernel in liblincheck.so, the parent commit's build "
                "against this one's (same compiler, same flags): VGPRs, SGPRs, LDS bytes, private segment bytes, "
                "VGPR and SGPR spill counts",
        "parent_kernels": len(parent),
        "head_kernels": len(head),
        "kernels_of_the_parent_that_differ": sorted(k for k in parent if head.get(k) != parent[k]),
        "new_kernels": {k: head[k] for k in sorted(head) if k not in parent},
        "units_of_the_parent_whose_device_text_differs": sorted(u for u in ptext if htext.get(u) != ptext[u]),
        "device_text_sha256": {u: {"parent": ptext[u], "head": htext.get(u)} for u in sorted(ptext)},
        "kernels": {k: {"parent": parent[k], "head": head.get(k), "same": head.get(k) == parent[k]} for k in sorted(parent)},
    }
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(parent)} parent kernels, {len(head)} head kernels, "
          f"{len(doc['kernels_of_the_parent_that_differ'])} differ, "
          f"{len(doc['units_of_the_parent_whose_device_text_differs'])} of {len(ptext)} units' device text differs, "
          f"new: {sorted(doc['new_kernels'])}")
    return 1 if doc["kernels_of_the_parent_that_differ"] else 0


if __name__ == "__main__":
    if len(sys.argv) != 4:
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
