#!/usr/bin/env python3
"""Times a multi-channel live session (vbx_session_open_channels / vbx_session_push_channels) on one MI355X: 16-bit PCM in pinned
host memory, 1200 / 480 at 48 kHz, every part on.  All times are a host clock around pushes that END IN vbx_sync (the upload and the
wait are part of what is measured); the two sides of every comparison alternate in one process after a warm-up, and the spread of the
passes (median of --runs passes of --pushes pushes, min - max of the passes) is reported with each median.

  small   n_sel in {1, 2, 8, 64} channels (all of the stream's) against 1, 10 and 100 hops per push: the multi-channel session's
          round trip against n_sel ONE-channel sessions on the same context pushed the same blocks -- the only form a caller had
          before -- with the ratio, the real-time factor and whether both sides wrote the same bits;
  large   8 channels of --hours of audio in 250,000-frame blocks against vbx_analyze_host_channels at chunk_frames = 250000 on the
          same bytes; the first and last 4,096 rows of every channel are compared as bits;
  alternating   64 channels, pushes of 1 and 5 hops in turn: the plane pitch Q -- and with it the segment list of the frame-loop call
          -- changes with EVERY push, so every push uploads the list anew through the context's one pinned staging buffer and waits
          on the host for the previous upload of it; each kind of push is timed against the same kind in a steady schedule, whose
          list repeats and is not uploaded;
  --trace HOPS --channels C   only a warmed run of --pushes multi-channel pushes, meant to run on its own under
          `rocprofv3 --kernel-trace --stats`; --count-trace CSV then counts the kernel dispatches per push in that trace (no GPU
          work): the dispatches from the first of the last --pushes session_ingest_all launches on, divided by --pushes.

  python tools/session_channels_bench.py --out profiles/session_channels/report.json
  rocprofv3 --kernel-trace --stats -d DIR -o h1_c64 --output-format csv -- python tools/session_channels_bench.py --trace 1 --channels 64
  python tools/session_channels_bench.py --count-trace DIR/h1_c64_kernel_trace.csv --trace 1 --channels 64 --out profiles/session_channels/report.json"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SR, ORDER, N, H = 48000.0, 12, 1200, 480


def emit(rows, **r):
    print(json.dumps(r), flush=True)
    rows.append(r)


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "runs": len(v)}


def recording(pkg, vb, n, channels):
    """n sample frames of `channels` channels of 16-bit PCM in pinned host memory: the synthetic speech, every channel shifted and
    scaled on its own (tiled from one minute of it)"""
    d = vb.synth_speech(min(n, 60 * 48000) + 64 * 977, sample_offset=5 * 48000 + 321)
    x = d.numpy()
    d.free()
    m = x.size - 64 * 977
    pinned = vb.malloc_host((n, channels), np.int16)
    for c in range(channels):
        one = np.round(x[c * 977:c * 977 + m] * ((0.9 - 0.005 * c) * 32767.0)).astype(np.int16)
        for a in range(0, n, m):
            k = min(m, n - a)
            pinned[a:a + k, c] = one[:k]
    return pinned


def make_params(pkg):
    est = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    return pkg.AnalysisParams.make(SR, formant_order=ORDER, est_init=est), pkg.AnalysisExt.make(rms=True)


def small(pkg, vb, rows, args):
    params, ext = make_params(pkg)
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    ld = rec + (rec & 1)
    for K in args.n_sel:
        for hops in args.hops:
            pushes = args.pushes
            T = N + hops * H * pushes
            audio = recording(pkg, vb, T, K)
            F = pkg.frame_count(T, N, H)
            outs = [[vb.empty((F, ld)) for _ in range(K)] for _ in range(2)]
            sts = [[vb.empty((3, F), np.int32) for _ in range(K)] for _ in range(2)]
            mb = max(N, hops * H)
            multi = vb.session_channels(params, ext, None, format=pkg.SAMPLE_PCM16, channels=K, frame_len=N, stride=H, max_block=mb)
            ones = [vb.session(params, ext, None, format=pkg.SAMPLE_PCM16, channels=K, channel=c, frame_len=N, stride=H, max_block=mb) for c in range(K)]

            def push_multi(a, b):
                lo = multi.info()[1]
                multi.push(audio[a:b], out=[o.ptr + lo * ld * 8 for o in outs[0]], status=[s.ptr + lo * 4 for s in sts[0]], record_ld=ld, status_ld=F)

            def push_ones(a, b):
                for c, s in enumerate(ones):
                    lo = s.info()[1]
                    s.push(audio[a:b], out=outs[1][c].ptr + lo * ld * 8, status=sts[1][c].ptr + lo * 4, record_ld=ld, status_ld=F)

            def run(push, reset, times):
                reset()
                push(0, N)
                vb.sync()
                pos = N
                for _ in range(pushes):
                    t0 = time.perf_counter()
                    push(pos, pos + hops * H)
                    vb.sync()
                    times.append((time.perf_counter() - t0) * 1e3)
                    pos += hops * H
            sides = (("session_channels", push_multi, multi.reset), ("one_channel_sessions", push_ones, lambda: [s.reset() for s in ones]))
            per = {k: [] for k, _, _ in sides}
            for i in range(args.warmup + args.runs):
                for k, push, reset in sides:
                    t = []
                    run(push, reset, t)
                    if i >= args.warmup:
                        per[k].append(statistics.median(t))
            same = all(np.array_equal(np.ascontiguousarray(outs[0][c].numpy()[:, :rec]).view(np.uint64),
                                      np.ascontiguousarray(outs[1][c].numpy()[:, :rec]).view(np.uint64)) and
                       np.array_equal(sts[0][c].numpy(), sts[1][c].numpy()) for c in range(K))
            block_ms = hops * 1e3 * H / SR
            for k in per:
                m = statistics.median(per[k])
                emit(rows, case="small", side=k, n_sel=K, hops_per_push=hops, pushes=pushes, **spread(per[k]),
                     real_time_factor=round(block_ms / m, 2), block_ms=round(block_ms, 3), completes_inside_its_block=bool(m < block_ms))
            s, b = statistics.median(per["session_channels"]), statistics.median(per["one_channel_sessions"])
            noise = max(max(v) - min(v) for v in per.values())
            emit(rows, case="small", side="verdict", n_sel=K, hops_per_push=hops, multi_over_one_channel_sessions=round(s / b, 4),
                 larger_spread_ms=round(noise, 4), not_slower_beyond_spread=bool(s - b <= noise), faster_beyond_spread=bool(b - s > noise),
                 same_bits=bool(same))
            multi.close()
            for s_ in ones:
                s_.close()
            for d in [x for side in outs + sts for x in side]:
                d.free()
            vb.free_host(audio)


def alternating(pkg, vb, rows, args):
    params, ext = make_params(pkg)
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    ld = rec + (rec & 1)
    K, kinds, pushes = 64, (1, 5), args.pushes
    T = N + sum(kinds) * H * pushes
    audio = recording(pkg, vb, T, K)
    F = pkg.frame_count(T, N, H)
    outs, sts = [vb.empty((F, ld)) for _ in range(K)], [vb.empty((3, F), np.int32) for _ in range(K)]
    q = {h: pkg.session_channels_plan(N + 80 * H, 0, h * H, N, H, 2, K)[0].plane_frames for h in kinds}
    assert q[1] != q[5], q
    sess = vb.session_channels(params, ext, None, format=pkg.SAMPLE_PCM16, channels=K, frame_len=N, stride=H, max_block=N + 80 * H)

    def run(schedule, times):
        sess.reset()
        lo = 0
        sess.push(audio[:N + 80 * H], out=outs, status=sts, record_ld=ld, status_ld=F)     # the warm-up saturates: every push analyses 64 + its own frames
        vb.sync()
        pos = N + 80 * H
        for hops in schedule:
            lo = sess.info()[1]
            t0 = time.perf_counter()
            sess.push(audio[pos:pos + hops * H], out=[o.ptr + lo * ld * 8 for o in outs], status=[s.ptr + lo * 4 for s in sts], record_ld=ld, status_ld=F)
            vb.sync()
            times.setdefault(hops, []).append((time.perf_counter() - t0) * 1e3)
            pos += hops * H
    n_each = (pushes - 80) // 2
    scheds = {"alternating": [1, 5] * (n_each // 2), "steady_1": [1] * n_each, "steady_5": [5] * (n_each // 3)}
    per = {}
    for i in range(args.warmup + args.runs):
        for name, sched in scheds.items():
            t = {}
            run(sched, t)
            if i >= args.warmup:
                for hops, v in t.items():
                    per.setdefault((name, hops), []).append(statistics.median(v))
    for hops in kinds:
        a, b = per[("alternating", hops)], per[("steady_%d" % hops, hops)]
        emit(rows, case="alternating", side="push_of_%d_hops" % hops, n_sel=K, hops_per_push=hops, plane_frames=q[hops],
             list_changes_every_push=spread(a), list_repeats=spread(b), added_ms=round(statistics.median(a) - statistics.median(b), 4),
             larger_spread_ms=round(max(max(a) - min(a), max(b) - min(b)), 4))
    sess.close()
    for d in outs + sts:
        d.free()
    vb.free_host(audio)


def large(pkg, vb, rows, args):
    params, ext = make_params(pkg)
    K = 8
    T = int(3600.0 * args.hours * SR)
    audio = recording(pkg, vb, T, K)
    F = pkg.frame_count(T, N, H)
    block = 250_000 * H
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    ld = rec + (rec & 1)
    outs, sts = [vb.empty((F, ld)) for _ in range(K)], [vb.empty((3, F), np.int32) for _ in range(K)]
    sess = vb.session_channels(params, ext, None, format=pkg.SAMPLE_PCM16, channels=K, frame_len=N, stride=H, max_block=min(block, T))

    def session_run():
        sess.reset()
        pos = 0
        while pos < T:
            n = min(block, T - pos)
            lo = sess.info()[1]
            sess.push(audio[pos:pos + n], out=[o.ptr + lo * ld * 8 for o in outs], status=[s.ptr + lo * 4 for s in sts], record_ld=ld, status_ld=F)
            pos += n
        vb.sync()

    def host_run():
        vb.analyze_host_channels(audio, params, ext, None, chunk_frames=250_000, frame_len=N, stride=H, out=outs, record_ld=ld, status=sts)
        vb.sync()
    cases = {"session_channels_250k_blocks": session_run, "analyze_host_channels_250k_chunks": host_run}
    times = {k: [] for k in cases}
    for i in range(args.warmup + args.runs):
        for k, fn in cases.items():
            t0 = time.perf_counter()
            fn()
            if i >= args.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    rows_cmp = min(4096, F)
    session_run()
    head = [o.numpy_slice(0, rows_cmp * ld) for o in outs]
    tail = [o.numpy_slice((F - rows_cmp) * ld, rows_cmp * ld) for o in outs]
    host_run()
    same = all(np.array_equal(head[c].view(np.uint64), outs[c].numpy_slice(0, rows_cmp * ld).view(np.uint64)) and
               np.array_equal(tail[c].view(np.uint64), outs[c].numpy_slice((F - rows_cmp) * ld, rows_cmp * ld).view(np.uint64)) for c in range(K))
    for k in cases:
        emit(rows, case="large", side=k, channels=K, hours=args.hours, frames_per_channel=F, **spread(times[k]),
             real_time_factor=round(T / SR / (statistics.median(times[k]) * 1e-3), 1))
    s, h = statistics.median(times["session_channels_250k_blocks"]), statistics.median(times["analyze_host_channels_250k_chunks"])
    noise = max(max(v) - min(v) for v in times.values())
    emit(rows, case="large", side="verdict", session_over_host=round(s / h, 4), difference_ms=round(s - h, 4), larger_spread_ms=round(noise, 4),
         not_slower_beyond_spread=bool(s - h <= noise), first_and_last_4096_rows_of_every_channel_same_bits=bool(same))
    sess.close()
    for d in outs + sts:
        d.free()
    vb.free_host(audio)


def trace(pkg, vb, args):
    params, ext = make_params(pkg)
    hops, pushes, K = args.trace, args.pushes, args.channels
    T = N + hops * H * (2 * pushes)
    audio = recording(pkg, vb, T, K)
    F = pkg.frame_count(T, N, H)
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    ld = rec + (rec & 1)
    outs, sts = [vb.empty((F, ld)) for _ in range(K)], [vb.empty((3, F), np.int32) for _ in range(K)]
    with vb.session_channels(params, ext, None, format=pkg.SAMPLE_PCM16, channels=K, frame_len=N, stride=H, max_block=max(N, hops * H)) as sess:
        sess.push(audio[:N], out=outs, status=sts, record_ld=ld, status_ld=F)
        pos = N
        for _ in range(2 * pushes):                          # the first half warms, the second half is what --count-trace counts
            lo = sess.info()[1]
            sess.push(audio[pos:pos + hops * H], out=[o.ptr + lo * ld * 8 for o in outs], status=[s.ptr + lo * 4 for s in sts], record_ld=ld, status_ld=F)
            vb.sync()
            pos += hops * H
    print(json.dumps({"case": "trace", "n_sel": K, "hops_per_push": hops, "pushes_counted": pushes}), flush=True)


def count_trace(path, args, rows):
    with open(path) as f:
        disp = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in disp]
    ingests = [i for i, n in enumerate(names) if "session_ingest_all_kernel" in n]
    assert len(ingests) >= args.pushes, (len(ingests), args.pushes)
    tail = names[ingests[-args.pushes]:]
    by_name = {}
    for n in tail:
        m = re.search(r"([A-Za-z_0-9]+)(<[^()]*>)?\(", n.replace("(anonymous namespace)", ""))
        short = m.group(1) if m else n
        by_name[short] = by_name.get(short, 0) + 1
    emit(rows, case="launches", n_sel=args.channels, hops_per_push=args.trace, pushes=args.pushes,
         kernel_launches_per_push=round(len(tail) / args.pushes, 2), per_kernel={k: round(v / args.pushes, 2) for k, v in sorted(by_name.items())})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hours", type=float, default=1.0 / 6.0, help="large blocks: hours of audio per channel (ten minutes to one hour)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pushes", type=int, default=200, help="pushes per timed pass of a small-block case / counted in a trace")
    ap.add_argument("--n-sel", type=int, nargs="+", default=[1, 2, 8, 64])
    ap.add_argument("--hops", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--only", choices=["large", "small", "alternating"], default=None)
    ap.add_argument("--trace", type=int, default=None, metavar="HOPS")
    ap.add_argument("--channels", type=int, default=64, help="channels of a --trace run")
    ap.add_argument("--count-trace", default=None, metavar="CSV")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    if args.count_trace:
        count_trace(args.count_trace, args, rows)
    else:
        import __graft_entry__ as g
        pkg = g.load_package()
        with pkg.VoxBox(0) as vb:
            if args.trace is not None:
                trace(pkg, vb, args)
            else:
                if args.only in (None, "small"):
                    small(pkg, vb, rows, args)
                if args.only in (None, "large"):
                    large(pkg, vb, rows, args)
                if args.only in (None, "alternating"):
                    alternating(pkg, vb, rows, args)
    if args.out and rows:
        kept = []
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
            key = lambda r: (r.get("case"), r.get("side"), r.get("n_sel"), r.get("hops_per_push"))
            new = {key(r) for r in rows}
            kept = [r for r in old if key(r) not in new]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(kept + rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
