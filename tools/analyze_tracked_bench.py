#!/usr/bin/env python3
"""Times the tracked frame loop against the sequence of calls it replaces, on the bench's utterance (1200 / 480 at 48 kHz,
4.5 M frames = 12.5 h, every part on), with HIP events on the context's stream, median of --runs calls after a warm-up:

  tracked    vbx_analyze_frames_tracked_f64 (kmax, Praat's path costs), and vbx_analyze_frames_tracked_pcm16 on 16-bit PCM;
  sequence   what a caller needs without it: vbx_analyze_frames_f64 + vbx_pitch_f64(kmax) + vbx_frame_peak_f64 +
             vbx_pitch_path_f64; on PCM: vbx_pcm16_to_f64 into a caller-owned copy, then the same four calls.  Also
             vbx_pitch_f64(kmax = 1) alone: the pass the fusion removes.

`sequence` uses nothing newer than the pitch path, so it runs from an older checkout too: --root DIR loads that tree's package
(build it first) -- the baseline of a comparison is the sequence built from the PARENT commit, not from the code under test.
One JSON line per case; --out FILE also writes the list of all of them; --merge A B .. --out FILE concatenates such lists (every
row names the checkout it was timed from in "root") into one report, without touching a GPU.

  python tools/analyze_tracked_bench.py --what tracked --out profiles/analyze_tracked/tracked.json
  python tools/analyze_tracked_bench.py --what sequence --root ../parent_checkout --out profiles/analyze_tracked/sequence.json
  python tools/analyze_tracked_bench.py --merge profiles/analyze_tracked/{tracked,sequence}.json --out profiles/analyze_tracked/report.json"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, SR = 1200, 480, 48000.0


def load_package(root):
    spec = importlib.util.spec_from_file_location("graft_entry_of_" + str(abs(hash(root))), os.path.join(root, "__graft_entry__.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g.load_package()


def median_ms(vb, fn, warmup, runs):
    for _ in range(warmup):
        fn()
    vb.sync()
    ms = []
    for _ in range(runs):
        vb.timer_begin()
        fn()
        ms.append(vb.timer_end())
    return statistics.median(ms), ms


def make_pcm(vb, F, piece_frames=450_000):
    """16-bit PCM of the whole view on the device: one synthesized piece, quantised on the host, tiled."""
    ns = (F - 1) * H + N
    piece = min(piece_frames * H, ns)
    tmp = vb.synth_speech(piece, sample_offset=0, sample_rate=SR)
    s = np.clip(np.rint(tmp.numpy() * 20000.0), -32768, 32767).astype(np.int16)
    tmp.free()
    pcm = vb.empty(ns, np.int16)
    for off in range(0, ns, piece):
        n = min(piece, ns - off)
        vb._check(vb.L.vbx_memcpy_h2d(vb.ctx, pcm.ptr + 2 * off, s.ctypes.data, 2 * n))
    return pcm


def report(rows, **r):
    r["frames_per_s"] = r["frames"] / (r["ms"] * 1e-3)
    r["ms"] = round(r["ms"], 3)
    r["all_ms"] = [round(v, 3) for v in r["all_ms"]]
    print(json.dumps(r), flush=True)
    rows.append(r)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=["tracked", "sequence", "both"], default="both")
    ap.add_argument("--root", default=HERE, help="the checkout whose built package is timed (default: this one)")
    ap.add_argument("--frames", type=int, default=4_500_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kmax", type=int, nargs="*", default=[4, 15])
    ap.add_argument("--no-pcm", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None, metavar="JSON", help="concatenate the row lists of earlier --out files into --out")
    args = ap.parse_args()
    if args.merge:
        assert args.out, "--merge needs --out"
        rows = []
        for path in args.merge:
            with open(path) as f:
                rows += json.load(f)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
        return
    assert args.runs >= 1
    pkg = load_package(os.path.abspath(args.root))
    F, rows = args.frames, []
    with pkg.VoxBox(0) as vb:
        name, cus = vb.device_info() if hasattr(vb, "device_info") else ("", 0)
        params = pkg.AnalysisParams.make(SR)
        REC = int(vb.L.vbx_record_doubles(params))
        REC += REC & 1
        ns = (F - 1) * H + N
        audio = vb.synth_speech(ns, sample_offset=0, sample_rate=SR)
        rec, st3 = vb.empty((F, REC)), vb.empty((3, F), np.int32)
        pcm = None if args.no_pcm else make_pcm(vb, F)
        common = dict(frames=F, frame_len=N, stride=H, root=os.path.basename(os.path.abspath(args.root)), device=name)

        if args.what in ("tracked", "both"):
            for kmax in args.kmax:
                track = pkg.PitchTrackParams.make(kmax=kmax)

                def f64():
                    vb.analyze_frames_tracked(audio, params, track, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=REC, status=st3)
                ms, all_ms = median_ms(vb, f64, args.warmup, args.runs)
                report(rows, case="tracked_f64", kmax=kmax, ms=ms, all_ms=all_ms, chunks_redone=vb.last_path_chunks_redone(), **common)
                vb.profile(True); vb.profile_reset(); f64()
                kern = {k: round(v[0], 3) for k, v in vb.profile_report().items()}
                vb.profile(False)
                print(json.dumps(dict(case="tracked_f64_kernels", kmax=kmax, kernels_ms=kern)), flush=True)
                rows.append(dict(case="tracked_f64_kernels", kmax=kmax, kernels_ms=kern, root=common["root"]))
                if pcm is not None:
                    def p16():
                        vb.analyze_frames_tracked_pcm16(pcm, params, track, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=REC,
                                                        status=st3)
                    ms, all_ms = median_ms(vb, p16, args.warmup, args.runs)
                    report(rows, case="tracked_pcm16", kmax=kmax, ms=ms, all_ms=all_ms, **common)

        if args.what in ("sequence", "both"):
            win = vb.window(pkg.WINDOW_HANNING, N)
            pk, path, idx = vb.empty(F), vb.empty((F, 2)), vb.empty(F, np.int32)
            cnt, pst = vb.empty(F, np.int32), vb.empty(F, np.int32)
            pp = pkg.PitchPathParams.make(time_step=H / SR)
            c1 = vb.empty((F, 1, 2))

            def pitch1():
                vb.pitch(audio, SR, 0.2, 75.0, 600.0, kmax=1, frame_len=N, stride=H, n_frames=F, window=win, out=(c1, cnt, pst))
            ms, all_ms = median_ms(vb, pitch1, args.warmup, args.runs)
            report(rows, case="pitch_kmax1_alone", kmax=1, ms=ms, all_ms=all_ms, **common)

            def plain():
                vb.analyze_frames(audio, params, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=REC, status=st3)
            ms, all_ms = median_ms(vb, plain, args.warmup, args.runs)
            report(rows, case="analyze_frames_alone", kmax=1, ms=ms, all_ms=all_ms, **common)
            c1.free()
            wide = None if pcm is None else vb.empty(ns)
            for kmax in args.kmax:
                cand = vb.empty((F, kmax, 2))

                def seq(x):
                    vb.analyze_frames(x, params, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=REC, status=st3)
                    vb.pitch(x, SR, 0.2, 75.0, 600.0, kmax=kmax, frame_len=N, stride=H, n_frames=F, window=win, out=(cand, cnt, pst))
                    vb.frame_peak(x, frame_len=N, stride=H, n_frames=F, out=pk)
                    vb.pitch_path(cand, cnt, pst, pk, params=pp, n_frames=F, kmax=kmax, out=(path, idx))
                ms, all_ms = median_ms(vb, lambda: seq(audio), args.warmup, args.runs)
                report(rows, case="sequence_f64", kmax=kmax, ms=ms, all_ms=all_ms, **common)
                if pcm is not None:
                    def seq16():
                        vb._check(vb.L.vbx_pcm16_to_f64(vb.ctx, pcm.ptr, ns, wide.ptr))
                        seq(wide)
                    ms, all_ms = median_ms(vb, seq16, args.warmup, args.runs)
                    report(rows, case="sequence_pcm16_widened", kmax=kmax, ms=ms, all_ms=all_ms, **common)
                cand.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
