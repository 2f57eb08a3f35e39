#!/usr/bin/env python3
"""Times the pitch path stage alone (vbx_pitch_path_f64), on lists vbx_pitch_f64 computed once beforehand:

  * the bench's single utterance (1200 / 480 at 48 kHz, 4.5 M frames = 12.5 h) at kmax 4, 15 and 63;
  * the same frames as 10,000 utterances of 450 frames;
  * a stream built to defeat forgetting (two near-equal tracks half an octave apart, tests/test_gpu_pitch_path.py);
  * the sequential form (chunk_frames >= F) once, for scale.

Prints one JSON line per case: frames/s, ms per call, chunks redone.  Run on an MI355X:  python tools/pitch_path_bench.py"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(vb, fn, warmup, steps):
    for _ in range(warmup):
        fn()
    vb.sync()
    vb.timer_begin()
    for _ in range(steps):
        fn()
    return vb.timer_end() / steps


def lists(vb, pkg, F, kmax, piece=450_000):
    N, H, SR = 1200, 480, 48000.0
    cand, cnt, st, pk = vb.empty((F, kmax, 2)), vb.empty(F, np.int32), vb.empty(F, np.int32), vb.empty(F)
    win = vb.window(pkg.WINDOW_HANNING, N)
    piece = min(piece, F)
    audio = vb.empty((piece - 1) * H + N)
    for p0 in range(0, F, piece):
        n = min(piece, F - p0)
        vb.synth_speech((n - 1) * H + N, sample_offset=p0 * H, out=audio)
        vb.pitch(audio, SR, 0.2, 75.0, 600.0, kmax=kmax, frame_len=N, stride=H, n_frames=n, window=win,
                 out=(cand.ptr + p0 * kmax * 16, cnt.ptr + p0 * 4, st.ptr + p0 * 4))
        vb.frame_peak(audio, frame_len=N, stride=H, n_frames=n, out=pk.ptr + p0 * 8)
    audio.free()
    return cand, cnt, st, pk


def adversarial(F, seed=3):
    """Two tracks half an octave apart whose score difference is a random walk far inside the switching cost: the non-leader's
    D keeps the whole history, so every chunk's warm-up guess is wrong (the same stream as tests/test_gpu_pitch_path.py)."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1e-4, 1e-4, F)
    cand = np.zeros((F, 2, 2))
    cand[:, 0] = np.stack([np.full(F, 200.0), 0.7 + d / 2], axis=-1)
    cand[:, 1] = np.stack([np.full(F, 200.0 * 2 ** 0.5), 0.7 - d / 2 - 0.005], axis=-1)
    return cand, np.full(F, 2, np.int32)


def case(vb, pkg, name, bufs, F, kmax, seg, steps, warmup, chunk_frames=0, silence=0.03):
    cand, cnt, st, pk = bufs
    params = pkg.PitchPathParams.make(chunk_frames=chunk_frames, silence_threshold=silence)
    path, idx = vb.empty((F, 2)), vb.empty(F, np.int32)

    def run():
        vb.pitch_path(cand, cnt, st, pk, seg_start=seg, params=params, n_frames=F, kmax=kmax, out=(path, idx))
    ms = timed(vb, run, warmup, steps)
    redone = vb.last_path_chunks_redone()
    vb.profile(True)                                           # one more call, with every kernel timed (events cost a little)
    vb.profile_reset()
    run()
    kernels = {k: round(v[0], 4) for k, v in vb.profile_report().items()}
    vb.profile(False)
    voiced = float(np.mean(idx.numpy() >= 0))
    path.free(); idx.free()
    r = dict(name=name, frames=F, kmax=kmax, segments=1 if seg is None else int(len(seg)), chunk_frames=chunk_frames,
             ms_per_call=round(ms, 4), frames_per_s=F / (ms * 1e-3), chunks_redone=redone, voiced_frac=round(voiced, 4), kernels_ms=kernels)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4_500_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kmax", type=int, nargs="*", default=[4, 15, 63])
    ap.add_argument("--no-sequential", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    F = args.frames
    with pkg.VoxBox(0) as vb:
        for kmax in args.kmax:
            t0 = time.time()
            bufs = lists(vb, pkg, F, kmax)
            vb.sync()
            print(json.dumps(dict(name="lists", kmax=kmax, seconds=round(time.time() - t0, 2))), flush=True)
            case(vb, pkg, "utterance", bufs, F, kmax, None, args.steps, args.warmup)
            case(vb, pkg, "10000x450", bufs, F, kmax, np.arange(0, F, 450, dtype=np.int64), args.steps, args.warmup)
            if kmax == args.kmax[0] and not args.no_sequential:
                case(vb, pkg, "utterance_sequential", bufs, F, kmax, None, 1, 0, chunk_frames=F)
            for b in bufs:
                b.free()
        # the adversarial stream: every warm-up guess is wrong
        Fa = 1_000_000
        cand, count = adversarial(Fa)
        bufs = (vb.to_device(cand), vb.to_device(count), None, None)
        case(vb, pkg, "adversarial", bufs, Fa, 2, None, args.steps, args.warmup, silence=0.0)
        for b in bufs[:2]:
            b.free()


if __name__ == "__main__":
    main()
