#!/usr/bin/env python3
"""float32 frames, LPC without MFCC (analyze_kernel<true, false, true, 0, 3, float>) and the same on f64 with the generic instance forced:
ms per call (best of four) per library build, one process per line.
usage: python3 tools/experiments/f32_lpc_ab.py lib/a.so lib/b.so [...]"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD = r'''
import sys, json, numpy as np
sys.path.insert(0, %(root)r)
import __graft_entry__ as g
pkg = g.load_package(); vb = pkg.VoxBox(0)
SR = 48000.0; ns = int(1.0 * 3600 * SR); audio = vb.synth_speech(ns)
x32 = vb.to_device(audio.numpy().astype(np.float32), np.float32)
n, hop = 1200, 480; F = pkg.frame_count(ns, n, hop); res = {}
params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=0, mfcc=None)
REC = (int(vb.L.vbx_record_doubles(params)) + 1) & ~1
rec = vb.empty((F, REC)); st3 = vb.empty((3, F), np.int32)
for label, fn, x in (("f32in lpc", vb.analyze_frames_ex_f32in, x32), ("f64 lpc", vb.analyze_frames, audio)):
    best = 1e30
    for _ in range(4):
        vb.timer_begin(); fn(x, params, frame_len=n, stride=hop, n_frames=F, out=rec, record_ld=REC, status=st3); best = min(best, vb.timer_end())
    res[label] = [best, F / best / 1e3]
print("RESULT " + json.dumps(res))
'''
for lib in sys.argv[1:]:
    env = dict(os.environ, VBX_LIB_PATH=os.path.abspath(lib), VBX_SPECTRAL_SPEC="0")
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        print(lib, "FAILED", p.stderr[-1500:]); sys.exit(1)
    r = json.loads(line[0][7:])
    print("%-28s %s" % (os.path.basename(lib), "  ".join("1200/480 %s %.2f ms %.2f M" % (k, v[0], v[1]) for k, v in r.items())), flush=True)
