#!/usr/bin/env python3
"""Gate 0 of the fused Burg lag sums (profiles/burg_fused/gate.txt): what does Burg's lag kernel cost the fused call?
One hour at 1200/480 through vbx_analyze_frames_f64, alternating rounds, one process per run, best of five calls:
  (a) formant_order = 0          (b) the side stream stops behind burg_lags (a -DVBX_EXP_BURG_LAGS_ONLY build)          (c) the full call
usage: python3 tools/experiments/burg_gate.py lib/libvoxbox_hip.so lib/libvoxbox_hip_lagsonly.so [--rounds 5] [--hours 1]"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD = r'''
import sys, json, numpy as np
sys.path.insert(0, %(root)r)
import __graft_entry__ as g
pkg = g.load_package(); vb = pkg.VoxBox(0)
SR = 48000.0; N, H = 1200, 480; ns = int(%(hours)f * 3600 * SR); audio = vb.synth_speech(ns)
est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
F = pkg.frame_count(ns, N, H)
kw = dict(lpc_order=12, formant_order=%(order)d, mfcc=(13, 100.0, 8000.0))
if %(order)d: kw["est_init"] = est0
params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), **kw)
REC = (int(vb.L.vbx_record_doubles(params)) + 1) & ~1
rec = vb.empty((F, REC)); st3 = vb.empty((3, F), np.int32); best = 1e30
for _ in range(5):
    vb.timer_begin(); vb.analyze_frames(audio, params, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=REC, status=st3); best = min(best, vb.timer_end())
print("GATE_RESULT " + json.dumps([best, F]))
'''
def run(lib, order, hours):
    env = dict(os.environ, VBX_LIB_PATH=os.path.abspath(lib))
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "hours": hours, "order": order}], env=env, capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("GATE_RESULT ")]
    if not line: raise SystemExit("FAILED %s order %d (exit %s): %s" % (lib, order, p.returncode, p.stderr[-1500:]))
    return json.loads(line[0][12:])
def main():
    args = sys.argv[1:]; rounds = 5; hours = 1.0
    if "--rounds" in args: i = args.index("--rounds"); rounds = int(args[i + 1]); del args[i:i + 2]
    if "--hours" in args: i = args.index("--hours"); hours = float(args[i + 1]); del args[i:i + 2]
    full, lags_only = args
    t = {"a": [], "b": [], "c": []}; F = 0
    for r in range(rounds):
        for k, lib, order in (("a", full, 0), ("b", lags_only, 12), ("c", full, 12)):
            ms, F = run(lib, order, hours); t[k].append(ms)
        print("round %d: (a) %.3f ms  (b) %.3f ms  (c) %.3f ms" % (r + 1, t["a"][-1], t["b"][-1], t["c"][-1]), flush=True)
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: max(v) - min(v) for k, v in t.items()}
    print("frames %d; medians (a) %.3f (b) %.3f (c) %.3f ms; spreads (max - min) %.3f %.3f %.3f ms" % (F, med["a"], med["b"], med["c"], spread["a"], spread["b"], spread["c"]))
    print("per frame: (b) - (a) = %.2f ns = %.1f %% of (c);  (c) - (b) = %.2f ns = %.1f %% of (c);  (c) = %.2f ns" % (
        (med["b"] - med["a"]) * 1e6 / F, 100 * (med["b"] - med["a"]) / med["c"], (med["c"] - med["b"]) * 1e6 / F, 100 * (med["c"] - med["b"]) / med["c"], med["c"] * 1e6 / F))
main()
