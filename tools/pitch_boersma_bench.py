#!/usr/bin/env python3
"""Times vbx_pitch_boersma_f64 against vbx_pitch_f64 on the same frames in the same run: 720,000 frames of 1200 / 480 synthetic
audio at 48 kHz (the bench's signal: voiced stretches and one second of noise in five), kmax 1, 4 and 15.

Per kmax the two calls are run interleaved (boersma, reference, boersma, ...) after a warm-up, each repetition timed by events on
the context's stream; the line carries the median, the fastest and the slowest repetition of each.  vbx_pitch_f64 is the baseline:
it is the call whose rows this one replaces.  With VBX_BOERSMA_GROUP=64 in the environment the library refines one entry per
wavefront at every kmax, instead of four at a time (16 lanes each) from kmax 4 on; run the tool once with and once without to compare.

Prints one JSON line per kmax.  Run on an MI355X:  python tools/pitch_boersma_bench.py"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def once(vb, fn):
    vb.timer_begin()
    fn()
    return vb.timer_end()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=720_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kmax", type=int, nargs="*", default=[1, 4, 15])
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, H, SR = 1200, 480, 48000.0
    F = args.frames
    with pkg.VoxBox(0) as vb:
        audio = vb.synth_speech((F - 1) * H + N, sample_offset=0)
        win = vb.window(pkg.WINDOW_HANNING, N)
        for kmax in args.kmax:
            a = (vb.empty((F, kmax, 2)), vb.empty(F, np.int32), vb.empty(F, np.int32))
            b = (vb.empty((F, kmax, 2)), vb.empty(F, np.int32), vb.empty(F, np.int32))

            def boersma():
                vb.pitch_boersma(audio, SR, 0.2, 75.0, 600.0, kmax=kmax, frame_len=N, stride=H, n_frames=F, window=win, out=a)

            def reference():
                vb.pitch(audio, SR, 0.2, 75.0, 600.0, kmax=kmax, frame_len=N, stride=H, n_frames=F, window=win, out=b)
            for _ in range(args.warmup):
                boersma()
                reference()
            vb.sync()
            tb, tr = [], []
            for _ in range(args.reps):
                tb.append(once(vb, boersma))
                tr.append(once(vb, reference))
            cnt = a[1].numpy()
            mb, mr = statistics.median(tb), statistics.median(tr)
            print(json.dumps(dict(
                kmax=kmax, frames=F, group=os.environ.get("VBX_BOERSMA_GROUP", "16") if kmax >= 4 else "64", reps=args.reps,
                boersma_ms=dict(median=round(mb, 3), min=round(min(tb), 3), max=round(max(tb), 3)),
                reference_ms=dict(median=round(mr, 3), min=round(min(tr), 3), max=round(max(tr), 3)),
                boersma_frames_per_s=round(F / (mb * 1e-3)), reference_frames_per_s=round(F / (mr * 1e-3)),
                boersma_over_reference=round(mb / mr, 3), mean_count=round(float(cnt.mean()), 2), max_count=int(cnt.max()))), flush=True)
            for d in a + b:
                d.free()
        audio.free()


if __name__ == "__main__":
    main()
