#!/usr/bin/env python3
"""Times a live session (vbx_session_*) on one MI355X: 16-bit PCM in pinned host memory, 1200 / 480 at 48 kHz, every part on.  All
times are a host clock around pushes that END IN vbx_sync (the upload and the wait are part of what is measured); the two sides of
every comparison alternate in one process after a warm-up, and the spread of the repeats is reported with each median.

  large   one hour of audio pushed in 250,000-frame blocks, against vbx_analyze_host at chunk_frames = 250000 on the same bytes (the
          device work is the same plus the two small kernels: parity is the expectation);
  small   blocks of 1, 10 and 100 hops: milliseconds per push round trip, the real-time factor (audio seconds analysed per wall
          second), and the same for the only correct incremental form a caller could write before -- a pinned copy into a resident
          recording, vbx_analyze_frames_ex_pcm16 on frames [lo - 64, hi), vbx_track_stitch_f64 from row lo - 1, a device copy of the own
          rows -- hand-written here against the same library;
  --trace HOPS   only a warmed run of --pushes session pushes of HOPS hops each, meant to run on its own under
          `rocprofv3 --kernel-trace --stats`; --count-trace CSV then counts the kernel dispatches per push in that trace (no GPU work):
          the dispatches from the first of the last --pushes session_ingest launches on, divided by --pushes.

  python tools/session_bench.py --out profiles/session/report.json
  rocprofv3 --kernel-trace --stats -d DIR -o h1 --output-format csv -- python tools/session_bench.py --trace 1
  python tools/session_bench.py --count-trace DIR/h1_kernel_trace.csv --trace 1 --out profiles/session/report.json"""
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
SR, ORDER, N, H, WARM = 48000.0, 12, 1200, 480, 64
HIP_MEMCPY_D2D = 3


def emit(rows, **r):
    print(json.dumps(r), flush=True)
    rows.append(r)


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "runs": len(v)}


def recording(pkg, vb, n):
    """n samples of the synthetic speech as 16-bit PCM in pinned host memory (tiled from one minute of it)"""
    d = vb.synth_speech(min(n, 60 * 48000), sample_offset=5 * 48000 + 321)
    one = np.round(d.numpy() * (0.9 * 32767.0)).astype(np.int16)
    d.free()
    pinned = vb.malloc_host(n, np.int16)
    for a in range(0, n, one.size):
        m = min(one.size, n - a)
        pinned[a:a + m] = one[:m]
    return pinned


def make_params(pkg):
    est = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    return pkg.AnalysisParams.make(SR, formant_order=ORDER, est_init=est), pkg.AnalysisExt.make(rms=True)


def large(pkg, vb, rows, args):
    params, ext = make_params(pkg)
    audio = recording(pkg, vb, int(3600.0 * args.hours * SR))
    T = audio.size
    F = pkg.frame_count(T, N, H)
    block = 250_000 * H
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    ld = rec + (rec & 1)
    out, st = vb.empty((F, ld)), vb.empty((3, F), np.int32)
    sess = vb.session(params, ext, None, format=pkg.SAMPLE_PCM16, frame_len=N, stride=H, max_block=block)

    def session_run():
        sess.reset()
        pos = 0
        while pos < T:
            n = min(block, T - pos)
            lo = sess.info()[1]
            sess.push(audio[pos:pos + n], out=out.ptr + lo * ld * 8, status=st.ptr + lo * 4, record_ld=ld, status_ld=F)
            pos += n
        vb.sync()

    def host_run():
        vb.analyze_host(audio, params, ext, None, chunk_frames=250_000, frame_len=N, stride=H, out=out, record_ld=ld, status=st)
        vb.sync()
    cases = {"session_250k_blocks": session_run, "analyze_host_250k_chunks": host_run}
    times = {k: [] for k in cases}
    for i in range(args.warmup + args.runs):
        for k, fn in cases.items():
            t0 = time.perf_counter()
            fn()
            if i >= args.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    # the two write the same bits (a slice is compared: the session's rows against the host call's)
    session_run()
    a = out.numpy_slice(0, 4096 * ld)
    b_tail = out.numpy_slice((F - 4096) * ld, 4096 * ld)
    host_run()
    same = bool(np.array_equal(a.view(np.uint64), out.numpy_slice(0, 4096 * ld).view(np.uint64)) and
                np.array_equal(b_tail.view(np.uint64), out.numpy_slice((F - 4096) * ld, 4096 * ld).view(np.uint64)))
    for k in cases:
        emit(rows, case="large", side=k, hours=args.hours, frames=F, **spread(times[k]),
             real_time_factor=round(T / SR / (statistics.median(times[k]) * 1e-3), 1))
    s, h = statistics.median(times["session_250k_blocks"]), statistics.median(times["analyze_host_250k_chunks"])
    noise = max(max(v) - min(v) for v in times.values())
    emit(rows, case="large", side="verdict", session_over_host=round(s / h, 4), difference_ms=round(s - h, 4), larger_spread_ms=round(noise, 4),
         inside_spread=bool(abs(s - h) <= noise), first_and_last_4096_rows_same_bits=same)
    sess.close()
    for d in (out, st):
        d.free()
    vb.free_host(audio)


class Baseline:
    """the incremental form a caller could write before: a resident PCM recording that grows by pinned copies, the resident frame
    loop on [lo - 64, hi), the stitch from row lo - 1, a device copy of the own rows"""

    def __init__(self, pkg, vb, params, ext, total, F, ld, out, st):
        self.pkg, self.vb, self.params, self.ext, self.F, self.ld, self.out, self.st = pkg, vb, params, ext, F, ld, out, st
        self.dev = vb.empty(total, np.int16)
        self.c_rec, self.c_st = vb.empty((F, ld)), vb.empty((3, F), np.int32)
        self.hip = C.CDLL(pkg.LIB_PATH)                      # (symbols looked up through the library's own handle: the runtime it is linked against)
        self.hip.hipMemcpyAsync.restype, self.hip.hipMemcpyAsync.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        vb.L.vbx_internal_stream.restype, vb.L.vbx_internal_stream.argtypes = C.c_void_p, [C.c_void_p]
        self.stream = vb.L.vbx_internal_stream(vb.ctx)
        self.consumed = 0

    def reset(self):
        self.consumed = 0

    def push(self, block):
        vb, L, ld = self.vb, self.vb.L, self.ld
        n = block.size
        vb._check(L.vbx_memcpy_h2d(vb.ctx, self.dev.ptr + 2 * self.consumed, block.ctypes.data, 2 * n))
        lo, hi = self.pkg.frame_count(self.consumed, N, H), self.pkg.frame_count(self.consumed + n, N, H)
        self.consumed += n
        if hi == lo:
            return
        warm = min(lo, WARM)
        n_an = hi - lo + warm
        vb._check(L.vbx_analyze_frames_ex_pcm16(vb.ctx, self.dev.ptr + 2 * (lo - warm) * H, n_an, N, H, C.byref(self.params), C.byref(self.ext), None,
                                                None, 0, self.c_rec.ptr, ld, self.c_st.ptr, None))
        if lo > 0:
            vb._check(L.vbx_track_stitch_f64(vb.ctx, self.c_rec.ptr + 16, n_an, ld, warm, n_an, self.out.ptr + ((lo - 1) * ld + 2) * 8, None))
        assert self.hip.hipMemcpyAsync(self.out.ptr + lo * ld * 8, self.c_rec.ptr + warm * ld * 8, (hi - lo) * ld * 8, HIP_MEMCPY_D2D, self.stream) == 0
        for k in range(3):
            assert self.hip.hipMemcpyAsync(self.st.ptr + (k * self.F + lo) * 4, self.c_st.ptr + (k * n_an + warm) * 4, (hi - lo) * 4, HIP_MEMCPY_D2D,
                                           self.stream) == 0


def small(pkg, vb, rows, args):
    params, ext = make_params(pkg)
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    ld = rec + (rec & 1)
    for hops in (1, 10, 100):
        pushes = args.pushes
        T = N + hops * H * pushes
        audio = recording(pkg, vb, T)
        F = pkg.frame_count(T, N, H)
        out, st = vb.empty((F, ld)), vb.empty((3, F), np.int32)
        out_b, st_b = vb.empty((F, ld)), vb.empty((3, F), np.int32)
        sess = vb.session(params, ext, None, format=pkg.SAMPLE_PCM16, frame_len=N, stride=H, max_block=max(N, hops * H))
        base = Baseline(pkg, vb, params, ext, T, F, ld, out_b, st_b)

        def run_session(times):
            sess.reset()
            sess.push(audio[:N], out=out, status=st, record_ld=ld, status_ld=F)
            vb.sync()
            pos = N
            for _ in range(pushes):
                lo = sess.info()[1]
                t0 = time.perf_counter()
                sess.push(audio[pos:pos + hops * H], out=out.ptr + lo * ld * 8, status=st.ptr + lo * 4, record_ld=ld, status_ld=F)
                vb.sync()
                times.append((time.perf_counter() - t0) * 1e3)
                pos += hops * H

        def run_baseline(times):
            base.reset()
            base.push(audio[:N])
            vb.sync()
            pos = N
            for _ in range(pushes):
                t0 = time.perf_counter()
                base.push(audio[pos:pos + hops * H])
                vb.sync()
                times.append((time.perf_counter() - t0) * 1e3)
                pos += hops * H
        per = {"session": [], "baseline": []}
        for i in range(args.warmup + args.runs):
            for k, fn in (("session", run_session), ("baseline", run_baseline)):
                t = []
                fn(t)
                if i >= args.warmup:
                    per[k].append(statistics.median(t))
        same = bool(np.array_equal(np.ascontiguousarray(out.numpy()[:, :rec]).view(np.uint64), np.ascontiguousarray(out_b.numpy()[:, :rec]).view(np.uint64))
                    and np.array_equal(st.numpy(), st_b.numpy()))
        for k in per:
            m = statistics.median(per[k])
            emit(rows, case="small", side=k, hops_per_push=hops, pushes=pushes, **spread(per[k]),
                 real_time_factor=round(hops * H / SR / (m * 1e-3), 2), hop_ms=round(1e3 * H / SR, 3))
        s, b = statistics.median(per["session"]), statistics.median(per["baseline"])
        noise = max(max(v) - min(v) for v in per.values())
        emit(rows, case="small", side="verdict", hops_per_push=hops, session_over_baseline=round(s / b, 4), larger_spread_ms=round(noise, 4),
             session_not_slower_beyond_spread=bool(s - b <= noise), same_bits=same,
             keeps_up_with_one_live_stream=bool(s < hops * 1e3 * H / SR), round_trip_over_block_duration=round(s / (hops * 1e3 * H / SR), 4))
        sess.close()
        for d in (out, st, out_b, st_b, base.dev, base.c_rec, base.c_st):
            d.free()
        vb.free_host(audio)


def trace(pkg, vb, args):
    params, ext = make_params(pkg)
    hops, pushes = args.trace, args.pushes
    T = N + hops * H * (2 * pushes)
    audio = recording(pkg, vb, T)
    F = pkg.frame_count(T, N, H)
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    ld = rec + (rec & 1)
    out, st = vb.empty((F, ld)), vb.empty((3, F), np.int32)
    with vb.session(params, ext, None, format=pkg.SAMPLE_PCM16, frame_len=N, stride=H, max_block=max(N, hops * H)) as sess:
        sess.push(audio[:N], out=out, status=st, record_ld=ld, status_ld=F)
        pos = N
        for _ in range(2 * pushes):                          # the first half warms, the second half is what --count-trace counts
            lo = sess.info()[1]
            sess.push(audio[pos:pos + hops * H], out=out.ptr + lo * ld * 8, status=st.ptr + lo * 4, record_ld=ld, status_ld=F)
            vb.sync()
            pos += hops * H
    print(json.dumps({"case": "trace", "hops_per_push": hops, "pushes_counted": pushes}), flush=True)


def count_trace(path, args, rows):
    with open(path) as f:
        disp = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in disp]
    ingests = [i for i, n in enumerate(names) if "session_ingest_kernel" in n]
    assert len(ingests) >= args.pushes, (len(ingests), args.pushes)
    tail = names[ingests[-args.pushes]:]
    by_name = {}
    for n in tail:
        m = re.search(r"([A-Za-z_0-9]+)(<[^()]*>)?\(", n.replace("(anonymous namespace)", ""))
        short = m.group(1) if m else n
        by_name[short] = by_name.get(short, 0) + 1
    emit(rows, case="launches", hops_per_push=args.trace, pushes=args.pushes, kernel_launches_per_push=round(len(tail) / args.pushes, 2),
         per_kernel={k: round(v / args.pushes, 2) for k, v in sorted(by_name.items())})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pushes", type=int, default=200, help="pushes per timed pass of a small-block case / counted in a trace")
    ap.add_argument("--only", choices=["large", "small"], default=None)
    ap.add_argument("--trace", type=int, default=None, metavar="HOPS")
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
                if args.only in (None, "large"):
                    large(pkg, vb, rows, args)
                if args.only in (None, "small"):
                    small(pkg, vb, rows, args)
    if args.out and rows:
        kept = []
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
            key = lambda r: (r.get("case"), r.get("side"), r.get("hops_per_push"))
            new = {key(r) for r in rows}
            kept = [r for r in old if key(r) not in new]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(kept + rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
