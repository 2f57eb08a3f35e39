#!/usr/bin/env python3
"""Writes tests/golden/frames_dispatch.json, the launches and digests tests/test_gpu_frames_dispatch.py pins the frame loop's
dispatch by sample type to.  Record it on the PARENT of the change under test, never on the change itself: build the parent in a
scratch worktree (git worktree add <dir> <commit>; make -C <dir>/vox_box.rs_amd) and point VBX_LIB_PATH at its libvoxbox_hip.so --
the Python package is the same on both sides.
usage: VBX_LIB_PATH=<parent's libvoxbox_hip.so> python3 tools/record_frames_dispatch.py <parent commit> [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as g
import test_gpu_frames_dispatch as t


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", t.GOLDEN)
    pkg = g.load_package()
    with pkg.VoxBox(0) as vb:
        cells = t.compute_cells(vb, pkg)
    doc = {"what": "tests/test_gpu_frames_dispatch.py::compute_cells on the library of commit %s (the parent of the change that made "
                   "the frames' sample type one view), recorded by: VBX_LIB_PATH=<that commit's libvoxbox_hip.so> python3 "
                   "tools/record_frames_dispatch.py %s" % (commit, commit),
           "cells": cells}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(cells), "cells")


if __name__ == "__main__":
    main()
