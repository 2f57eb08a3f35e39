#!/usr/bin/env python3
"""Times vbx_analyze_clips on one MI355X: 16-bit PCM clips at 48 kHz in device memory, 1200 / 480, every part on.  All times are a
host clock around calls that END IN vbx_sync; the two sides of every comparison alternate in one process after a warm-up, and the
spread of the passes (median of --runs passes, min - max) is reported with each median.  Both sides write the same kind of arrays,
and their bits are compared.

  corpus  --clips clips of 1 to 10 s (uniform, fixed seed): ONE vbx_analyze_clips call against one vbx_analyze_frames_ex_pcm16 call
          per clip on the same context -- the only form a caller has without it -- plain and tracked (kmax 4), with the ratio;
  single  one clip of 100,000 frames against the resident call on it: what the pack, the staging rows and the deliver cost, which are
          an extra pass over the data by construction;
  --trace   only warmed corpus calls (plain), meant to run on its own under `rocprofv3 --kernel-trace --stats`; --count-trace CSV
          then reads that run's kernel stats (no GPU work) and reports the launches per group: every kernel's calls divided by the
          calls of clips_deliver_kernel.

  python tools/analyze_clips_bench.py --out profiles/analyze_clips/report.json
  rocprofv3 --kernel-trace --stats -d DIR -o corpus --output-format csv -- python tools/analyze_clips_bench.py --trace
  python tools/analyze_clips_bench.py --count-trace DIR/corpus_kernel_stats.csv --out profiles/analyze_clips/report.json"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SR, ORDER, N, H, KMAX = 48000.0, 12, 1200, 480, 4


def emit(rows, **r):
    print(json.dumps(r), flush=True)
    rows.append(r)


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "runs": len(v)}


def corpus(pkg, vb, lengths):
    """the clips back to back in ONE device buffer (each at its own 16-byte aligned offset), cut from a minute of the synthetic
    speech at its own shift and gain: (buffer, element offsets)"""
    d = vb.synth_speech(60 * 48000 + 4096 * 31, sample_offset=5 * 48000 + 321)
    x = d.numpy()
    d.free()
    offs, pos = [], 0
    for ln in lengths:
        offs.append(pos)
        pos += (ln + 7) & ~7
    image = np.zeros(pos, np.int16)
    for b, (o, ln) in enumerate(zip(offs, lengths)):
        s = (b % 4096) * 31
        image[o:o + ln] = np.round(x[s:s + ln] * ((0.9 - 0.0001 * (b % 4096)) * 32767.0)).astype(np.int16)
    return vb.to_device(image, np.int16), offs


class Outputs:
    def __init__(self, vb, total, ld, tracked):
        self.rec, self.st = vb.empty((total, ld)), vb.empty((3, total), np.int32)
        self.lists = (vb.empty((total, KMAX, 2)), vb.empty(total, np.int32), vb.empty(total), vb.empty(total, np.int32)) if tracked else None

    def arrays(self):
        return [self.rec, self.st] + (list(self.lists) if self.lists else [])

    def free(self):
        for a in self.arrays():
            a.free()


def compare(one, many, rec):
    """the one call's records and lists against the per-clip calls' (whose status rows are [3, n_rows] blocks: not compared)"""
    a, b = one.rec.numpy()[:, :rec], many.rec.numpy()[:, :rec]
    same = bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    if one.lists:
        for x, y in zip(one.lists, many.lists):
            u, v = x.numpy(), y.numpy()
            same = same and bool(np.array_equal(u.view(np.uint8), v.view(np.uint8)))
    return same


def run_corpus(pkg, vb, rows, args, tracked):
    rng = np.random.default_rng(2048)
    lengths = [int(v) for v in rng.integers(48000, 480001, args.clips)]
    est = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    params, ext = pkg.AnalysisParams.make(SR, formant_order=ORDER, est_init=est), pkg.AnalysisExt.make(rms=True)
    track = pkg.PitchTrackParams.make(kmax=KMAX) if tracked else None
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    ld = rec + (rec & 1)
    plan, total, groups = pkg.clips_plan(lengths, N, H)
    buf, offs = corpus(pkg, vb, lengths)
    one, many = Outputs(vb, total, ld, tracked), Outputs(vb, total, ld, tracked)
    st_tmp = vb.empty((3, max(int(plan[:, 1].max()), 1)), np.int32)             # (a per-clip call writes [3, n_rows]: not compared)
    n = len(lengths)
    h_clip = (C.c_void_p * n)(*[buf.ptr + 2 * o for o in offs])
    h_len = (C.c_size_t * n)(*lengths)
    cf = pkg.ClipFormat.make(pkg.SAMPLE_PCM16, args.group_frames)
    tk = None if track is None else C.byref(track)

    def outputs_at(o, r0):
        if o.lists is None:
            return None
        c, k, p, i = o.lists
        return C.byref(pkg.PitchTrackOutputs(c.ptr + r0 * KMAX * 16, k.ptr + r0 * 4, p.ptr + r0 * 8, i.ptr + r0 * 4))

    def call_one():
        vb._check(vb.L.vbx_analyze_clips(vb.ctx, h_clip, h_len, n, C.byref(cf), N, H, C.byref(params), C.byref(ext), tk, one.rec.ptr, ld,
                                         one.st.ptr, outputs_at(one, 0)))

    def call_many():
        for b in range(n):
            r0, nr = int(plan[b, 0]), int(plan[b, 1])
            if nr:
                vb._check(vb.L.vbx_analyze_frames_ex_pcm16(vb.ctx, buf.ptr + 2 * offs[b], nr, N, H, C.byref(params), C.byref(ext), tk, None, 0,
                                                           many.rec.ptr + r0 * ld * 8, ld, st_tmp.ptr, outputs_at(many, r0)))
    if args.trace:
        for _ in range(args.warmup + args.runs):
            call_one()
            vb.sync()
        return
    sides = (("analyze_clips", call_one), ("per_clip_calls", call_many))
    per = {k: [] for k, _ in sides}
    for i in range(args.warmup + args.runs):
        for k, call in sides:
            vb.sync()
            t0 = time.perf_counter()
            call()
            vb.sync()
            if i >= args.warmup:
                per[k].append((time.perf_counter() - t0) * 1e3)
    a, b = spread(per["analyze_clips"]), spread(per["per_clip_calls"])
    wider = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    emit(rows, case="corpus", form="tracked" if tracked else "plain", clips=n, frames=total, groups=groups, seconds_of_audio=round(sum(lengths) / SR, 1),
         analyze_clips=a, per_clip_calls=b, ratio=round(b["median_ms"] / a["median_ms"], 3),
         m_frames_per_s={"analyze_clips": round(total / a["median_ms"] / 1e3, 3), "per_clip_calls": round(total / b["median_ms"] / 1e3, 3)},
         faster_beyond_the_larger_spread=bool(b["median_ms"] - a["median_ms"] > wider), same_bits=compare(one, many, rec))
    for d in (buf, st_tmp):
        d.free()
    one.free(); many.free()


def run_single(pkg, vb, rows, args):
    F = 100_000
    ln = N + (F - 1) * H
    est = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    params, ext = pkg.AnalysisParams.make(SR, formant_order=ORDER, est_init=est), pkg.AnalysisExt.make(rms=True)
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    ld = rec + (rec & 1)
    buf, offs = corpus(pkg, vb, [48000 * 60] * (ln // (48000 * 60) + 1))          # (whole minutes back to back: one long recording)
    one, res = Outputs(vb, F, ld, False), Outputs(vb, F, ld, False)
    h_clip, h_len = (C.c_void_p * 1)(buf.ptr), (C.c_size_t * 1)(ln)
    cf = pkg.ClipFormat.make(pkg.SAMPLE_PCM16, args.group_frames)

    def call_one():
        vb._check(vb.L.vbx_analyze_clips(vb.ctx, h_clip, h_len, 1, C.byref(cf), N, H, C.byref(params), C.byref(ext), None, one.rec.ptr, ld,
                                         one.st.ptr, None))

    def call_res():
        vb._check(vb.L.vbx_analyze_frames_ex_pcm16(vb.ctx, buf.ptr, F, N, H, C.byref(params), C.byref(ext), None, None, 0, res.rec.ptr, ld,
                                                   res.st.ptr, None))
    sides = (("analyze_clips", call_one), ("resident_call", call_res))
    per = {k: [] for k, _ in sides}
    for i in range(args.warmup + args.runs):
        for k, call in sides:
            vb.sync()
            t0 = time.perf_counter()
            call()
            vb.sync()
            if i >= args.warmup:
                per[k].append((time.perf_counter() - t0) * 1e3)
    a, b = spread(per["analyze_clips"]), spread(per["resident_call"])
    same = bool(np.array_equal(one.rec.numpy()[:, :rec].view(np.uint64), res.rec.numpy()[:, :rec].view(np.uint64)) and
                np.array_equal(one.st.numpy(), res.st.numpy()))
    emit(rows, case="single", frames=F, groups=pkg.clips_plan([ln], N, H, args.group_frames)[2], analyze_clips=a, resident_call=b,
         extra_ms=round(a["median_ms"] - b["median_ms"], 4), ratio=round(a["median_ms"] / b["median_ms"], 3), same_bits=same)
    buf.free(); one.free(); res.free()


def count_trace(path, rows):
    calls = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            calls[r["Name"]] = calls.get(r["Name"], 0) + int(r["Calls"])
    groups = sum(v for k, v in calls.items() if "clips_deliver_kernel" in k)
    assert groups, "no clips_deliver_kernel in the trace"
    short = lambda k: k.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
    per = {}
    for k, v in calls.items():
        per[short(k)] = per.get(short(k), 0) + v
    emit(rows, case="launches", groups=groups, dispatches_per_group=round(sum(calls.values()) / groups, 2),
         per_group={k: round(v / groups, 3) for k, v in sorted(per.items(), key=lambda kv: -kv[1])})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--group-frames", type=int, default=0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--count-trace", metavar="CSV", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    if args.count_trace:
        count_trace(args.count_trace, rows)
    else:
        import __graft_entry__ as g
        pkg = g.load_package()
        with pkg.VoxBox(0) as vb:
            if args.trace:
                run_corpus(pkg, vb, rows, args, False)
            else:
                run_corpus(pkg, vb, rows, args, False)
                run_corpus(pkg, vb, rows, args, True)
                run_single(pkg, vb, rows, args)
    if args.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        old = []
        if args.count_trace and os.path.exists(args.out):
            old = [r for r in json.load(open(args.out)) if r.get("case") != "launches"]
        json.dump(old + rows, open(args.out, "w"), indent=1)
        open(args.out, "a").write("\n")


if __name__ == "__main__":
    main()
