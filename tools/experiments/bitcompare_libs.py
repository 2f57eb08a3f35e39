#!/usr/bin/env python3
"""Every column of the fused call's record, of vbx_pitch_f64 (kmax 1 and 8) and of vbx_find_formants_f64 (Burg rows, resonance rows,
tracks, statuses), bit for bit between two builds of the library, on an hour of the bench's recording at several frame shapes.
usage: python3 tools/experiments/bitcompare_libs.py lib/a.so lib/b.so [--hours 1]      (each build runs in a child process)

--tables: instead, one call per kind of host-built device table (the window, Goertzel, two-stage, matrix-core, chirp-z, interpolation,
DCT, slopes, bins, resample and f32 lag-window tables), 64 frames of the synthetic recording each, one child process per build and per
environment setting; every vbx_mfcc_f64 call must take the form tests/test_gpu_layouts.py lists for its shape."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(1200, 480), (1024, 512), (2048, 1024), (4096, 2048), (1103, 441), (800, 320), (512, 256)]

CHILD = r'''
import sys, json, hashlib, numpy as np
sys.path.insert(0, %(root)r)
import __graft_entry__ as g
pkg = g.load_package(); vb = pkg.VoxBox(0)
SR = 48000.0
ns = int(%(hours)f * 3600 * 48000)
audio = vb.synth_speech(ns)
est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
out = {}
def dig(a): return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
for n, hop in %(shapes)r:
    F = min(pkg.frame_count(ns, n, hop), 200000)
    params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=12, est_init=est0, mfcc=(13, 100.0, 8000.0))
    rec, st3 = vb.analyze_frames(audio, params, frame_len=n, stride=hop, n_frames=F)
    han = vb.window(pkg.WINDOW_HANNING, n)
    c1, n1, s1 = vb.pitch(audio, SR, 0.2, 75., 600., kmax=1, frame_len=n, stride=hop, n_frames=F, window=han)
    c8, n8, s8 = vb.pitch(audio, SR, 0.2, 75., 600., kmax=8, frame_len=n, stride=hop, n_frames=min(F, 50000), window=han)
    ff = vb.find_formants(audio, SR, 12, est0, frame_len=n, stride=hop, n_frames=F)
    cols = params.columns()
    d = {"frames": F, "status3": dig(st3), "pitch1": dig(c1), "count1": dig(n1), "pitch8": dig(c8)}
    for k, (c0, w) in cols.items(): d["record_" + k] = dig(rec[:, c0:c0 + w])
    for k in ("formants", "res", "count", "coeffs", "status"): d["ff_" + k] = dig(ff[k])
    out["%%d/%%d" %% (n, hop)] = d
print("BITCMP " + json.dumps(out))
'''

# (frame length, upper band edge, the form vbx_internal_last_mfcc_form must report: tests/test_gpu_layouts.py) per environment setting
TABLE_MFCC = {
    "": [(337, 8000.0, 6), (400, 8000.0, 4), (700, 8000.0, 4), (1000, 8000.0, 4), (1024, 8000.0, 1), (1200, 8000.0, 1), (2048, 8000.0, 1),
         (4096, 8000.0, 1), (1103, 8000.0, 2), (1103, 16000.0, 3), (5000, 8000.0, 7)],
    "VBX_MFCC_DFT2=1": [(1200, 8000.0, 5)],
    "VBX_MFCC_CZT_SPLIT=1": [(1103, 16000.0, 3)],                 # the two-block chirp-z tables
}

TABLES_CHILD = r'''
import sys, json, hashlib, numpy as np
sys.path.insert(0, %(root)r)
import __graft_entry__ as g
pkg = g.load_package(); vb = pkg.VoxBox(0)
SR, F = 48000.0, 64
out, wrong_form = {}, []
def dig(a): return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
def rec(n): hop = 2 * n // 5; return vb.synth_speech((F - 1) * hop + n), hop
for n, hi, form in %(mfcc)r:
    audio, hop = rec(n)
    mf, st = vb.mfcc(audio, 13, (100.0, hi), SR, frame_len=n, stride=hop, n_frames=F, window=vb.window(pkg.WINDOW_HANNING, n))
    got = int(vb.L.vbx_internal_last_mfcc_form(vb.ctx))
    if got != form: wrong_form.append([n, hi, form, got])
    out["mfcc-%%d-hi%%d" %% (n, hi)] = {"form": got, "mfcc": dig(mf), "status": dig(st)}
if %(rest)r:
    out["dct-13"] = {"rows": dig(vb.dct(np.random.default_rng(13).standard_normal((F, 13))))}
    est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    for n in (1200, 1024):
        audio, hop = rec(n)
        han = vb.window(pkg.WINDOW_HANNING, n)
        c, k, s = vb.pitch(audio, SR, 0.2, 75.0, 600.0, kmax=4, frame_len=n, stride=hop, n_frames=F, window=han)
        out["pitch_f64-%%d" %% n] = {"cand": dig(c), "count": dig(k), "status": dig(s)}
    audio, hop = rec(1200)
    for ratio in (0.5, 1.5):
        out["resample-1200-%%g" %% ratio] = {"rows": dig(vb.resample_linear(audio, ratio, frame_len=1200, stride=hop, n_frames=F))}
    x32 = np.lib.stride_tricks.sliding_window_view(audio.numpy(), 1200)[::hop][:F].astype(np.float32)
    c, k, s = vb.pitch_f32(x32, SR, 0.2, 75.0, 600.0, kmax=4, window=pkg.window_table(pkg.WINDOW_HANNING, 1200))
    out["pitch_f32-1200"] = {"cand": dig(c), "count": dig(k), "status": dig(s)}
    ff = vb.find_formants(audio, SR, 12, est0, frame_len=1200, stride=hop, n_frames=F)
    out["find_formants-1200"] = {k: dig(ff[k]) for k in ("formants", "res", "count", "coeffs", "status")}
    for n, hop in ((1200, 480), (1103, 441)):
        audio = vb.synth_speech((F - 1) * hop + n)
        params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=12, est_init=est0, mfcc=(13, 100.0, 8000.0))
        r, st3 = vb.analyze_frames(audio, params, frame_len=n, stride=hop, n_frames=F)
        d = {"status3": dig(st3), "mfcc_interp": int(vb.L.vbx_internal_last_mfcc_interp(vb.ctx))}
        for k, (c0, w) in params.columns().items(): d["record_" + k] = dig(r[:, c0:c0 + w])
        out["record-%%d/%%d" %% (n, hop)] = d
print("BITCMP " + json.dumps({"calls": out, "wrong_form": wrong_form}))
'''


def tables(libs):
    """-> the report; exit status 1 when a digest differs or a call did not take its intended form"""
    rep = {"mode": "tables", "libs": [os.path.basename(a) for a in libs], "frames": 64, "settings": {}}
    failed = False
    for setting, mfcc in TABLE_MFCC.items():
        res = []
        for lib in libs:
            env = dict(os.environ, VBX_LIB_PATH=os.path.abspath(lib))
            if setting:
                env[setting.split("=")[0]] = setting.split("=")[1]
            p = subprocess.run([sys.executable, "-c", TABLES_CHILD % {"root": ROOT, "mfcc": mfcc, "rest": setting == ""}], env=env,
                               capture_output=True, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith("BITCMP ")]
            if not line:
                print(lib, setting, "FAILED", p.stdout[-1500:], p.stderr[-1500:]); return 1
            res.append(json.loads(line[0][7:]))
        calls = {}
        for name, d in res[0]["calls"].items():
            diff = [k for k in d if any(r["calls"][name][k] != d[k] for r in res[1:])]
            calls[name] = dict(d, differs=diff)
            failed = failed or bool(diff)
            print(setting or "default", name, "IDENTICAL" if not diff else "DIFFER in %s" % diff)
        wrong = [r["wrong_form"] for r in res]
        failed = failed or any(wrong)
        rep["settings"][setting or "default"] = {"calls": calls, "calls_not_in_their_form": wrong}
    rep["verdict"] = "FAILED" if failed else "every digest identical, every vbx_mfcc_f64 call in its form"
    print("BITCMP_REPORT " + json.dumps(rep))
    return 1 if failed else 0


def main():
    args = sys.argv[1:]
    if "--tables" in args:
        args.remove("--tables")
        return tables(args)
    hours = 1.0
    if "--hours" in args:
        i = args.index("--hours"); hours = float(args[i + 1]); del args[i:i + 2]
    res = []
    for lib in args:
        env = dict(os.environ, VBX_LIB_PATH=os.path.abspath(lib))
        p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "hours": hours, "shapes": SHAPES}], env=env, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("BITCMP ")]
        if not line:
            print(lib, "FAILED", p.stdout[-1500:], p.stderr[-1500:]); return 1
        res.append(json.loads(line[0][7:]))
    rep = {"libs": [os.path.basename(a) for a in args], "hours": hours, "shapes": {}}
    for shape in res[0]:
        diff = [k for k in res[0][shape] if any(r[shape][k] != res[0][shape][k] for r in res[1:])]
        rep["shapes"][shape] = {"frames": res[0][shape]["frames"], "columns_compared": len(res[0][shape]) - 1, "columns_that_differ": diff}
        print(shape, res[0][shape]["frames"], "frames:", "IDENTICAL" if not diff else "DIFFER in %s" % diff)
    print("BITCMP_REPORT " + json.dumps(rep))
    return 0

sys.exit(main())
