#!/usr/bin/env python3
"""Writes tests/golden/front_end_once_digests.json, the digests tests/test_gpu_front_end_once.py pins the candidate front
end of the fused kernel to.  Run it only on a build whose outputs are the accepted ones (the library is the tree's, or VBX_LIB_PATH's).
usage: python3 tools/record_front_end_once_digests.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as g
import test_gpu_front_end_once as t


def main():
    pkg = g.load_package()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", t.GOLDEN)
    with pkg.VoxBox(0) as vb:
        digests = t.compute_digests(vb, pkg)
    doc = {"what": "sha-256 of the outputs of tests/test_gpu_front_end_once.py::compute_digests",
           "library": os.path.basename(os.environ.get("VBX_LIB_PATH") or "libvoxbox_hip.so"), "digests": digests}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
