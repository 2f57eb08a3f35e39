#!/usr/bin/env python3
"""Times the 8-bit sample formats (VBX_SAMPLE_U8 / ULAW / ALAW) against the 16-bit path of the SAME build on one MI355X.  Both sides
of every comparison ALTERNATE in one process after a warm-up; each case ends in vbx_sync and is timed on the host clock; reported are
the median of --runs passes with min and max.  Nothing is measured against the code under test alone:

  unpack          unpack_ulaw / unpack_alaw / unpack_u8 on 2^28 mono samples and unpack_all_ulaw on 8 channels (2^25 sample frames),
                  against unpack_pcm16 / unpack_all_pcm16 on the same element count: bytes read + written per second, and output
                  bytes per second (the G.711 decode should hide behind the stores: same output rate as PCM16, or say so);
  host recording  vbx_analyze_host on an hour of mu-law at 8 kHz (the golden WAV tiled, encoded to the nearest codes) from pinned
                  memory, against the same call on the same audio decoded to PCM16 beforehand (that decode is NOT timed; its numpy
                  time is reported as context).  The bar: not slower beyond the larger spread of the two sides;
  clip batch      vbx_analyze_clips on 2,048 mu-law clips of 1 to 10 s against the same clips as PCM16; the same bar.

  python tools/sample8_bench.py --out profiles/sample8/report.json"""
import argparse
import json
import os
import statistics
import sys
import time
import wave

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
HBM_ROOF_GBPS = 8000.0                  # MI355X: 8 TB/s
SR = 8000.0


def alternate(cases, warmup, runs):
    """cases: [fn], each ending in a synchronise.  Every case once per round, in order; the per-case lists of wall times (ms)."""
    for _ in range(warmup):
        for fn in cases:
            fn()
    ms = [[] for _ in cases]
    for _ in range(runs):
        for i, fn in enumerate(cases):
            t0 = time.perf_counter()
            fn()
            ms[i].append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(t):
    return dict(ms=round(statistics.median(t), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3), spread_ms=round(max(t) - min(t), 3))


def nearest_codes(table, s16):
    """the code whose table value is nearest to each 16-bit sample (numpy.searchsorted on the sorted table, as the tests do)"""
    t = table.astype(np.int64)
    order = np.argsort(t, kind="stable")
    ts = t[order]
    s = s16.astype(np.int64)
    i = np.clip(np.searchsorted(ts, s), 1, 255)
    i = np.where(np.abs(ts[i - 1] - s) <= np.abs(ts[i] - s), i - 1, i)
    return order[i].astype(np.uint8)


def golden():
    with wave.open(os.path.join(HERE, "tests", "golden", "sample-two_vowels.wav"), "rb") as w:
        a = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)
        return a.reshape(-1, w.getnchannels())[:, 0].copy()


def bench_unpack(pkg, vb, args, emit):
    n = 1 << args.log2_samples
    rng = np.random.default_rng(8)
    tile8 = rng.integers(0, 256, 1 << 24).astype(np.uint8)
    src8 = vb.to_device(np.resize(tile8, n), np.uint8)
    src16 = vb.to_device(np.resize(rng.integers(-32768, 32768, 1 << 24).astype(np.int16), n), np.int16)
    out = vb.empty(n)                                       # doubles: large enough for every plane type
    sel8 = np.arange(8, dtype=np.int32)
    mono = [("unpack_pcm16", pkg.SAMPLE_PCM16, src16, 2, 2), ("unpack_ulaw", pkg.SAMPLE_ULAW, src8, 1, 2), ("unpack_alaw", pkg.SAMPLE_ALAW, src8, 1, 2),
            ("unpack_u8", pkg.SAMPLE_U8, src8, 1, 8)]
    allc = [("unpack_all_pcm16", pkg.SAMPLE_PCM16, src16, 2, 2), ("unpack_all_ulaw", pkg.SAMPLE_ULAW, src8, 1, 2)]

    def one(fmt, src):
        def fn():
            vb._check(vb.L.vbx_unpack_samples(vb.ctx, src.ptr, n, fmt, 1, 0, out.ptr))
            vb.sync()
        return fn

    def eight(fmt, src):
        def fn():
            vb._check(vb.L.vbx_unpack_channels(vb.ctx, src.ptr, n // 8, fmt, 8, sel8.ctypes.data, 8, out.ptr, n // 8))
            vb.sync()
        return fn
    for group, cases, make in (("mono", mono, one), ("eight_channels", allc, eight)):
        ms = alternate([make(c[1], c[2]) for c in cases], args.warmup, args.runs)
        rows = {}
        for (name, _, _, sb, ob), t in zip(cases, ms):
            med = statistics.median(t) * 1e-3
            rows[name] = emit(case="unpack", kernel=name, layout=group, elements=n, bytes_in=n * sb, bytes_out=n * ob,
                              GBps=round(n * (sb + ob) / med / 1e9, 1), out_GBps=round(n * ob / med / 1e9, 1),
                              out_GBps_best=round(n * ob / (min(t) * 1e-3) / 1e9, 1), out_GBps_worst=round(n * ob / (max(t) * 1e-3) / 1e9, 1),
                              fraction_of_hbm_roof=round(n * (sb + ob) / med / 1e9 / HBM_ROOF_GBPS, 3), all_ms=[round(x, 3) for x in t], **stats(t))
        ref = rows[cases[0][0]]
        for name in [c[0] for c in cases[1:] if c[4] == 2]:
            r = rows[name]
            allowed = max(r["spread_ms"], ref["spread_ms"])
            emit(case="unpack_bar", kernel=name, against=ref["kernel"], ms=r["ms"], against_ms=ref["ms"], allowed_ms=allowed,
                 decode_hidden_behind_the_stores=bool(r["ms"] <= ref["ms"] + allowed))
    for d in (src8, src16, out):
        d.free()


def analysis_shape(pkg, vb, params):
    """200 / 80 (25 ms / 10 ms at 8 kHz) where the resident PCM16 call accepts it, else the smallest shape that it does"""
    probe = np.zeros(4000, np.int16)
    for shape in ((200, 80), (400, 160), (1200, 480)):
        try:
            vb.analyze_frames_ex_pcm16(probe, params, None, None, frame_len=shape[0], stride=shape[1])
            return shape
        except pkg.VoxBoxError:
            continue
    raise SystemExit("no shape accepted")


def bench_host(pkg, vb, args, emit, params, shape, table):
    N, H = shape
    n = int(args.hours * 3600 * SR)
    t0 = time.perf_counter()
    codes_np = nearest_codes(table, np.resize(golden(), n))
    t_encode = time.perf_counter() - t0
    codes = vb.malloc_host(n, np.uint8)
    codes[:] = codes_np
    t0 = time.perf_counter()
    decoded = table[codes_np]
    t_decode = (time.perf_counter() - t0) * 1e3
    pcm = vb.malloc_host(n, np.int16)
    pcm[:] = decoded
    F = pkg.frame_count(n, N, H)
    rec = int(vb.L.vbx_record_doubles(params)); rec += rec & 1
    out, st = vb.empty((F, rec)), vb.empty((3, F), np.int32)

    def side(audio, fmt):
        def fn():
            vb.analyze_host(audio, params, format=fmt, frame_len=N, stride=H, out=out, record_ld=rec, status=st)
            vb.sync()
        return fn
    ms = alternate([side(codes, pkg.SAMPLE_ULAW), side(pcm, None)], args.warmup, args.runs)
    common = dict(hours=args.hours, sample_rate=SR, frames=F, frame_len=N, stride=H, pinned=True)
    a = emit(case="host_recording", format="ulaw", bytes_uploaded=n, frames_per_s=round(F / (statistics.median(ms[0]) * 1e-3)),
             all_ms=[round(x, 3) for x in ms[0]], **stats(ms[0]), **common)
    b = emit(case="host_recording", format="pcm16_decoded_beforehand", bytes_uploaded=2 * n, frames_per_s=round(F / (statistics.median(ms[1]) * 1e-3)),
             all_ms=[round(x, 3) for x in ms[1]], **stats(ms[1]), **common)
    allowed = max(a["spread_ms"], b["spread_ms"])
    emit(case="host_recording_bar", ulaw_ms=a["ms"], pcm16_ms=b["ms"], allowed_ms=allowed, met=bool(a["ms"] <= b["ms"] + allowed),
         host_numpy_decode_ms_not_timed_above=round(t_decode, 1), host_numpy_encode_s_test_input_only=round(t_encode, 1), **common)
    # the same bits: the two sides' records
    side(pcm, None)()
    want = out.numpy_slice(0, min(F, 100_000) * rec).view(np.int64)
    side(codes, pkg.SAMPLE_ULAW)()
    emit(case="host_recording_bits_equal", equal=bool(np.array_equal(out.numpy_slice(0, min(F, 100_000) * rec).view(np.int64), want)),
         frames_compared=min(F, 100_000))
    vb.free_host(codes); vb.free_host(pcm)
    out.free(); st.free()


def bench_clips(pkg, vb, args, emit, params, shape, table):
    N, H = shape
    rng = np.random.default_rng(2048)
    lengths = rng.integers(int(SR), int(10 * SR) + 1, args.clips).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    total_samples = int(lengths.sum())
    codes_np = nearest_codes(table, np.resize(golden(), total_samples))
    d_codes, d_pcm = vb.to_device(codes_np, np.uint8), vb.to_device(table[codes_np], np.int16)
    _, total, groups = pkg.clips_plan(lengths.tolist(), N, H)
    rec = int(vb.L.vbx_record_doubles(params)); rec += rec & 1
    out, st = vb.empty((total, rec)), vb.empty((3, total), np.int32)

    def side(dev, fmt, es):
        ptrs = [dev.ptr + int(o) * es for o in offs]

        def fn():
            vb.analyze_clips(ptrs, lengths.tolist(), params, format=fmt, frame_len=N, stride=H, out=out, record_ld=rec, status=st)
            vb.sync()
        return fn
    ms = alternate([side(d_codes, pkg.SAMPLE_ULAW, 1), side(d_pcm, pkg.SAMPLE_PCM16, 2)], args.warmup, args.runs)
    common = dict(clips=args.clips, samples=total_samples, rows=total, groups=groups, frame_len=N, stride=H, sample_rate=SR)
    a = emit(case="clip_batch", format="ulaw", all_ms=[round(x, 3) for x in ms[0]], **stats(ms[0]), **common)
    b = emit(case="clip_batch", format="pcm16", all_ms=[round(x, 3) for x in ms[1]], **stats(ms[1]), **common)
    allowed = max(a["spread_ms"], b["spread_ms"])
    emit(case="clip_batch_bar", ulaw_ms=a["ms"], pcm16_ms=b["ms"], allowed_ms=allowed, met=bool(a["ms"] <= b["ms"] + allowed), **common)
    for d in (d_codes, d_pcm, out, st):
        d.free()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log2-samples", type=int, default=28, help="mono samples of the unpack cases (2^28 = 256 M)")
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--only", default="unpack,host,clips")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    rows = []

    def emit(**r):
        print(json.dumps(r), flush=True)
        rows.append(r)
        return r
    only = set(args.only.split(","))
    with pkg.VoxBox(0) as vb:
        name, cus = vb.device_info()
        emit(case="device", device=name, compute_units=cus, runs=args.runs, warmup=args.warmup)
        if "unpack" in only:
            bench_unpack(pkg, vb, args, emit)
        params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 500.0), mfcc=(13, 100.0, 3800.0))
        table = pkg.g711_table(pkg.SAMPLE_ULAW)
        if only & {"host", "clips"}:
            shape = analysis_shape(pkg, vb, params)
            emit(case="shape", frame_len=shape[0], stride=shape[1], sample_rate=SR)
        if "host" in only:
            bench_host(pkg, vb, args, emit, params, shape, table)
        if "clips" in only:
            bench_clips(pkg, vb, args, emit, params, shape, table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
