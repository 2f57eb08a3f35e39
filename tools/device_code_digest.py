#!/usr/bin/env python3
"""Per-kernel digests of a unit's device assembly, independent of the order the compiler emitted the kernels in.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/UNIT.hip -o UNIT.s
    tools/device_code_digest.py UNIT.s [...]          # one line per kernel: sha256 of its text, its symbol; sorted by symbol

A host-side refactor must leave every line as it was: same symbols, same text.  What is normalised away, and only that: the order of
the kernels in the file (it follows the order in which the host code names them), the function's ordinal in its local labels
(.LBB<ordinal>_<block>, .Lfunc_end<ordinal>, the comments that name them and the blanks that pad those comments), and the compilation unit's id symbol (__hip_cuid_<hash of the source path>).
The kernels' entries of the metadata note are digested the same way (sorted), as the line `<sha256> <unit>: metadata`.
"""
import hashlib
import re
import sys

ORDINAL = re.compile(r"\.?(LBB|BB|Lfunc_end|Lfunc_begin|Ltmp)\d+(?=_|\b)")
PAD = re.compile(r"[ \t]+;")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
SECTION = re.compile(r"^\t\.section\t\.text\.(\S+?),")


def norm(line):
    line = CUID.sub("__hip_cuid_X", ORDINAL.sub(lambda m: m.group(1) + "N", line))
    return PAD.sub(" ;", line)                           # (a label's comment column moves with the ordinal's digits)


def digest(path):
    chunks, key, meta, in_meta = {}, None, [], False
    for raw in open(path, errors="replace"):
        line = norm(raw)
        if line.startswith("\t.amdgpu_metadata"):
            in_meta, key = True, None
        if in_meta:
            meta.append(line)
            continue
        m = SECTION.match(line)
        if m:
            key = m.group(1)
        elif line.startswith("\t.section\t.AMDGPU.gpr_maximums"):
            key = None                                   # the unit's trailer follows whichever kernel came last
        chunks.setdefault(key or "(unit)", []).append(line)
    out = [(hashlib.sha256("".join(v).encode()).hexdigest(), k) for k, v in chunks.items()]
    # the metadata note: one YAML item per kernel under amdhsa.kernels, each starting at "  - "
    items, cur = [], []
    for line in meta:
        if (line.startswith("  - ") or line.startswith("amdhsa.")) and cur:
            items.append("".join(cur)); cur = []
        cur.append(line)
    items.append("".join(cur))
    out.append((hashlib.sha256("".join(sorted(items)).encode()).hexdigest(), "metadata"))
    return sorted(out, key=lambda t: t[1])


if __name__ == "__main__":
    for p in sys.argv[1:]:
        unit = p.rsplit("/", 1)[-1]
        for h, k in digest(p):
            print(h, unit + ": " + k)
