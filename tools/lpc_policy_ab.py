"""A/B of the LPC policies (VBX_LPC_POLICY_EXACT / PLAIN / REFERENCE, include/voxbox_hip.h), timed with vbx_timer_*; prints ONE
JSON line.  Shapes:
  pipeline   vbx_analyze_frames_f64 at 48 kHz 1200 / 480 (pitch + LPC(12) + find_formants(12) + MFCC(13)), the bench.py flagship
  config2    vbx_autocorr_lpc_f64 on dense 512-sample Hanning frames, order 12
  speech13   vbx_analyze_frames_f64 at 44.1 kHz 1103 / 441, LPC(13) only (the order whose LPC runs beside the fused kernel)
Run each invocation on the GPU under its own time limit (timeout -k 10 ...)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def _time(vb, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    vb.sync()
    ms = []
    for _ in range(steps):
        vb.timer_begin()
        fn()
        ms.append(vb.timer_end())
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pipeline-frames", type=int, default=200_000)
    ap.add_argument("--dense-frames", type=int, default=1_000_000)
    ap.add_argument("--speech-frames", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    pkg = ge.load_package()
    policies = {"exact": pkg.LPC_POLICY_EXACT, "plain": pkg.LPC_POLICY_PLAIN, "reference": pkg.LPC_POLICY_REFERENCE}
    out = {"metric": "frames_per_s", "shapes": {}}
    with pkg.VoxBox(0) as vb:
        n, hop, F = 1200, 480, a.pipeline_frames
        audio = vb.synth_speech((F - 1) * hop + n, sample_offset=0)
        est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
        prm = pkg.AnalysisParams.make(48000.0, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=12, est_init=est0,
                                      mfcc=(13, 100.0, 8000.0))
        rec = vb.empty((F, _record_ld(vb, prm)))
        res = {}
        for name, pol in policies.items():
            vb.lpc_policy = pol
            ms = _time(vb, lambda: vb.analyze_frames(audio, prm, frame_len=n, stride=hop, n_frames=F, out=rec), a.steps, a.warmup)
            res[name] = F / (ms * 1e-3)
        out["shapes"]["pipeline_1200_480"] = res
        rec.free(); audio.free()

        F = a.dense_frames
        audio = vb.synth_speech(F * 512, sample_offset=0)
        han = vb.window(pkg.WINDOW_HANNING, 512)
        r, lp = vb.empty((F, 13)), vb.empty((F, 13))
        res = {}
        for name, pol in policies.items():
            vb.lpc_policy = pol
            ms = _time(vb, lambda: vb.autocorr_lpc(audio, 12, frame_len=512, stride=512, n_frames=F, window=han, out=(r, lp)),
                       a.steps, a.warmup)
            res[name] = F / (ms * 1e-3)
        out["shapes"]["config2_512_p12"] = res
        r.free(); lp.free(); audio.free()

        n, hop, F = 1103, 441, a.speech_frames
        audio = vb.synth_speech((F - 1) * hop + n, sample_offset=0, sample_rate=44100.0)
        prm = pkg.AnalysisParams.make(44100.0, pitch=(0.2, 75.0, 600.0), lpc_order=13, formant_order=0, mfcc=(0, 100.0, 8000.0))
        rec = vb.empty((F, _record_ld(vb, prm)))
        res = {}
        for name, pol in policies.items():
            vb.lpc_policy = pol
            ms = _time(vb, lambda: vb.analyze_frames(audio, prm, frame_len=n, stride=hop, n_frames=F, out=rec), a.steps, a.warmup)
            res[name] = F / (ms * 1e-3)
        out["shapes"]["analyze_1103_441_p13"] = res
        rec.free(); audio.free()
    for s in out["shapes"].values():
        s["reference_over_exact"] = s["reference"] / s["exact"]
    print(json.dumps(out))


def _record_ld(vb, prm):
    rec = int(vb.L.vbx_record_doubles(C.byref(prm)))
    return rec + (rec & 1)                                   # what VoxBox.analyze_frames passes as record_ld


if __name__ == "__main__":
    main()
