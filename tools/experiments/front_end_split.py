#!/usr/bin/env python3
"""The candidate front end of the headline analyze kernel, stage by stage, from counter passes of builds that stop early.

  front_end_split.py run              the driver of one counter pass (rocprofv3 --pmc ... -- python3 front_end_split.py run): the fused
                                      call (no formants) at 1200 / 480 on ten minutes of the bench's recording, on its voiced seconds
                                      only and on its unvoiced seconds only (the split of pitch_by_signal.py), each ONCE and in this
                                      order, so that the per-dispatch counter rows can be told apart
  front_end_split.py table DIR        the table: DIR/<variant>/ holds the counter csv files of one build each (front_end_split.sh);
                                      variants are full_parent, full_new, p1..p6 (the plain form stopped by -DVBX_EXP_STOP=k) and
                                      n2..n6 (the form that computes each value once; it differs from the filter on: stop 1 is
                                      the same code in both forms, so p1 serves both)
Stages are differences of stopped forms: scan = stop 1 - transforms (the known 3.1 k are not separated here: `scan` includes them),
filter = 2 - 1, prefix = 3 - 2, bounds = 4 - 3, first pick = 5 - 4, store = 6 - 4, Brent loop and later picks = full - 5 - store."""
import collections
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIGNALS = ("bench mix", "voiced seconds", "unvoiced seconds")
COUNTERS = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVE_CYCLES")


def run():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package(); vb = pkg.VoxBox(0)
    N, H, SR, secs = 1200, 480, 48000.0, 600
    mix = vb.synth_speech(secs * 48000).numpy()
    sec = (np.arange(mix.size) // 48000) % 5
    voiced = mix[sec != 4]
    noise = mix[sec == 4]
    params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=0, mfcc=(13, 100.0, 8000.0))
    for name, sig in zip(SIGNALS, (mix, voiced, noise)):
        d = vb.to_device(np.ascontiguousarray(sig))
        F = pkg.frame_count(sig.size, N, H)
        vb.analyze_frames(d, params, frame_len=N, stride=H, n_frames=F)
        vb.sync()
        print(name, F, "frames", flush=True)
        d.free()


def read_variant(path):
    """-> [per signal] {counter: value per wave} of the analyze kernel's dispatches, in dispatch order"""
    rows = collections.OrderedDict()
    for fn in glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(fn)):
            if "analyze_kernel" not in r["Kernel_Name"]:
                continue
            rows.setdefault(int(r["Dispatch_Id"]), {})[r["Counter_Name"]] = float(r["Counter_Value"])
    out = []
    for _, v in sorted(rows.items()):
        w = v["SQ_WAVES"]
        out.append(dict({c: v[c] / w for c in COUNTERS}, waves=w))
    return out


def table(d):
    got = {os.path.basename(p): read_variant(p) for p in sorted(glob.glob(os.path.join(d, "*"))) if os.path.isdir(p)}
    got = {k: v for k, v in got.items() if len(v) == len(SIGNALS)}
    fmt = lambda r: "VALU %8.1f  SALU %7.1f  LDS %6.1f  wave cycles %8.0f" % tuple(r[c] for c in COUNTERS)
    sub = lambda a, b: {c: a[c] - b[c] for c in COUNTERS}
    for si, sname in enumerate(SIGNALS):
        v = {k: r[si] for k, r in got.items()}
        print("== %s (%d frames), per frame" % (sname, int(next(iter(v.values()))["waves"])))
        for k in sorted(v):
            print("  %-12s %s" % (k, fmt(v[k])))
        for form, full in (("p", "full_parent"), ("n", "full_new")):
            s = lambda k: v.get("p1") if k == 1 else v.get(form + str(k))    # the peak scan is the same code in both forms
            missing = [form + str(k) for k in range(1, 7) if s(k) is None]
            if full not in v or missing:
                print("  stages of %s: not shown, no counters of %s" % (full, " ".join(missing) or full))
                continue
            print("  stages of %s:" % full)
            print("    transforms + LPC / MFCC rows + peak scan  %s" % fmt(s(1)))
            for name, a, b in (("filter", 2, 1), ("prefix sums", 3, 2), ("bounds", 4, 3), ("first pick", 5, 4), ("store (last evaluation to the end)", 6, 4)):
                print("    %-42s %s" % (name, fmt(sub(s(a), s(b)))))
            rest = sub(sub(v[full], s(5)), sub(s(6), s(4)))
            print("    %-42s %s" % ("Brent evaluations + later picks", fmt(rest)))
            fe = sub(sub(s(5), s(1)), {c: 0.0 for c in COUNTERS})
            print("    %-42s %s" % ("front end (filter .. first pick)", fmt(fe)))
        if "full_parent" in v and "full_new" in v:
            print("  full_new - full_parent                      %s" % fmt(sub(v["full_new"], v["full_parent"])))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "table":
        table(sys.argv[2])
    else:
        run()
