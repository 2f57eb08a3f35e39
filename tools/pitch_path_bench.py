#!/usr/bin/env python3
"""Times the pitch path stage alone (vbx_pitch_path_f64), on lists vbx_pitch_f64 computed once beforehand:

  * the bench's single utterance (1200 / 480 at 48 kHz, 4.5 M frames = 12.5 h) at kmax 4, 15 and 63;
  * the same frames as 10,000 utterances of 450 frames;
  * a stream built to defeat forgetting (two near-equal tracks half an octave apart, tests/test_gpu_pitch_path.py);
  * the sequential form (chunk_frames >= F) once, for scale.

With --shards N (one or more values) the utterance is also run through the shard hand-off (vbx_pitch_path_shard_begin_f64 / _enter /
_finish) with ONE device playing N ranks, one context per rank: per rank the time of each of the three calls beside the plain call
on the same frames, the chunks redone, and whether the stitched rows equal the whole call's.

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


def shard_case(pkg, vb, bufs, F, kmax, world, steps, warmup):
    """The utterance through the hand-off, one context per played rank; the lists are slices of the whole recording's."""
    cand, cnt, st, pk = bufs
    params = pkg.PitchPathParams.make()
    whole_p, whole_i = vb.empty((F, 2)), vb.empty(F, np.int32)
    vb.pitch_path(cand, cnt, st, pk, params=params, n_frames=F, kmax=kmax, out=(whole_p, whole_i))
    want_p, want_i = whole_p.numpy(), whole_i.numpy()
    whole_p.free(); whole_i.free()
    ctxs = [pkg.VoxBox(0) for _ in range(world)]
    plans = [pkg.shard_plan(F, world, r) for r in range(world)]
    one = np.array([0], np.int64)
    rk = []
    for c, pl in zip(ctxs, plans):
        a, n = pl.lo - pl.warm, pl.hi - pl.lo + pl.warm
        rk.append(dict(a=a, n=n, cand=cand.ptr + a * kmax * 16, cnt=cnt.ptr + a * 4, st=st.ptr + a * 4, pk=pk.ptr + a * 8,
                       path=c.empty((n, 2)), idx=c.empty(n, np.int32), state=c.empty(64), back=c.empty(64, np.int32),
                       changed=c.empty(1, np.int32), end=c.empty(1, np.int32), spk=c.empty(1)))
    peak = np.fmax.reduce([c.pitch_path_segment_peaks(d["pk"], d["n"]) for c, d in zip(ctxs, rk)])
    for c, d in zip(ctxs, rk):
        c.L.vbx_memcpy_h2d(c.ctx, d["spk"].ptr, peak.ctypes.data, 8)

    def begin(r):
        c, d, pl = ctxs[r], rk[r], plans[r]
        c.pitch_path_shard_begin(d["cand"], d["cnt"], d["st"], d["n"], kmax, d["pk"], d["spk"], one, params, pl.warm,
                                 pl.continues_prev, pl.continues_next)

    def enter(r):
        ctxs[r].pitch_path_shard_enter(rk[r - 1]["state"] if plans[r].continues_prev else None, rk[r]["state"], rk[r]["back"],
                                       rk[r]["changed"])

    def finish(r):
        ctxs[r].pitch_path_shard_finish(rk[r]["end"] if plans[r].continues_next else None, rk[r]["path"], 2, rk[r]["idx"])

    out = []
    for r in range(world):                                     # begin, timed; its own repairs
        ms_b = timed(ctxs[r], lambda: begin(r), warmup, steps)
        out.append(dict(rank=r, frames=rk[r]["n"], begin_ms=round(ms_b, 4), begin_chunks_redone=ctxs[r].last_path_chunks_redone()))
    for r in range(world):                                     # enter in rank order: the first call repairs, the timed ones find it done
        enter(r)
        ctxs[r].sync()
        out[r]["enter_chunks_redone"] = int(rk[r]["changed"].numpy()[0])
        out[r]["enter_ms"] = round(timed(ctxs[r], lambda: enter(r), warmup, steps), 4)
    ends = pkg.shard.path_end_states([d["back"].numpy() for d in rk], plans)
    for r in range(world):
        if ends[r] is not None:
            ctxs[r].L.vbx_memcpy_h2d(ctxs[r].ctx, rk[r]["end"].ptr, np.array([ends[r]], np.int32).ctypes.data, 4)
        out[r]["finish_ms"] = round(timed(ctxs[r], lambda: finish(r), warmup, steps), 4)
        out[r]["shard_ms"] = round(out[r]["begin_ms"] + out[r]["enter_ms"] + out[r]["finish_ms"], 4)
    got_p = np.concatenate([d["path"].numpy()[pl.warm:] for d, pl in zip(rk, plans)])
    got_i = np.concatenate([d["idx"].numpy()[pl.warm:] for d, pl in zip(rk, plans)])
    equal = bool(np.array_equal(got_i, want_i) and np.array_equal(got_p.view(np.int64), want_p.view(np.int64)))
    for r in range(world):                                     # the plain call on the same frames, on the same context
        c, d = ctxs[r], rk[r]
        out[r]["plain_ms"] = round(timed(c, lambda: c.pitch_path(d["cand"], d["cnt"], d["st"], d["pk"], params=params, n_frames=d["n"],
                                                                 kmax=kmax, out=(d["path"], d["idx"])), warmup, steps), 4)
    for c, d in zip(ctxs, rk):
        for k in ("path", "idx", "state", "back", "changed", "end", "spk"):
            d[k].free()
        c.close()
    r = dict(name="shards", world=world, frames=F, kmax=kmax, equals_whole_call=equal, ranks=out,
             shard_ms_max=max(o["shard_ms"] for o in out), plain_ms_max=max(o["plain_ms"] for o in out),
             enter_chunks_redone=sum(o["enter_chunks_redone"] for o in out))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4_500_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kmax", type=int, nargs="*", default=[4, 15, 63])
    ap.add_argument("--no-sequential", action="store_true")
    ap.add_argument("--no-adversarial", action="store_true")
    ap.add_argument("--no-segments", action="store_true", help="skip the 10,000 x 450 case")
    ap.add_argument("--shards", type=int, nargs="*", default=[], help="also run the utterance through the shard hand-off at these world sizes")
    ap.add_argument("--root", default=ROOT, help="the checkout whose library is timed (default: this one; a build of the parent commit for an A/B)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
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
            if not args.no_segments:
                case(vb, pkg, "10000x450", bufs, F, kmax, np.arange(0, F, 450, dtype=np.int64), args.steps, args.warmup)
            for world in args.shards:
                shard_case(pkg, vb, bufs, F, kmax, world, args.steps, args.warmup)
            if kmax == args.kmax[0] and not args.no_sequential:
                case(vb, pkg, "utterance_sequential", bufs, F, kmax, None, 1, 0, chunk_frames=F)
            for b in bufs:
                b.free()
        if args.no_adversarial:
            return
        # the adversarial stream: every warm-up guess is wrong
        Fa = 1_000_000
        cand, count = adversarial(Fa)
        bufs = (vb.to_device(cand), vb.to_device(count), None, None)
        case(vb, pkg, "adversarial", bufs, Fa, 2, None, args.steps, args.warmup, silence=0.0)
        for b in bufs[:2]:
            b.free()


if __name__ == "__main__":
    main()
