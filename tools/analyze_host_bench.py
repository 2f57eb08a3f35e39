#!/usr/bin/env python3
"""Times vbx_analyze_host against the host-fed pattern a caller had to write before it, on the bench's 1200 / 480 pipeline (48 kHz,
every part on) over a 16-bit PCM recording in pinned host memory, on one MI355X.  The cases ALTERNATE in one process, median of
--runs after a warm-up, each case closed by a synchronise and timed on the host clock (the uploads are part of what is measured):

  (a) host_call        this build's vbx_analyze_host at the default chunk_frames, the recording cut into 1,000-frame utterances;
  (b) pattern_parent   the build under --root (the PARENT commit's) running the loop INTEGRATION.md documented until now -- the loop
                       of bench.py's bench_host_fed: two device buffers, a copy stream, ready / freed events, chunks of whole
                       1,000-frame utterances, vbx_analyze_frames_pcm16 per chunk -- driven from Python through the HIP runtime;
  (c) host_call_one    (a) on ONE long utterance (no segment list): every cut is stitched;
  (d) resident_pcm16   this build's vbx_analyze_frames_ex_pcm16 on the same recording already resident (no upload in the loop).

The bar: (a) is not slower than (b) by more than the larger of the two cases' spreads.  Also reported: (a) / (d), device memory in use
(hipMemGetInfo) with the host call's buffers against the resident recording, a slice of (a)'s records against (d)'s bit for bit, and
-- with --unpack, meant to be run on its own under `rocprofv3 --kernel-trace --stats` -- each unpack_* kernel's bytes per second.

--out FILE keeps the rows of the OTHER mode that FILE already holds (the bench rows replace bench rows, the unpack rows replace unpack
rows), so the three steps below build one report; --merge-trace CSV adds the per-dispatch times of that run's kernel trace to the
unpack rows (trace_*: dispatches 1-5 of a kernel are its mono launches, 6-10 its stereo ones, as --unpack issues them):

  python tools/analyze_host_bench.py --root ../parent_checkout --out profiles/analyze_host/report.json
  rocprofv3 --kernel-trace --stats -d DIR -o unpack --output-format csv -- \
      python tools/analyze_host_bench.py --unpack --out profiles/analyze_host/report.json
  python tools/analyze_host_bench.py --merge-trace DIR/unpack_kernel_trace.csv --out profiles/analyze_host/report.json
  (DIR/unpack_kernel_trace.csv and DIR/unpack_kernel_stats.csv are kept beside the report)"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, ORDER, N, H, SEG_FRAMES = 48000.0, 12, 1200, 480, 1000
PKG_NAME = "vox_box_rs_amd"
HBM_ROOF_GBPS = 8000.0                  # MI355X: 8 TB/s
HIP_MEMCPY_H2D, HIP_STREAM_NON_BLOCKING, HIP_EVENT_DISABLE_TIMING = 1, 1, 2


def load_package(root):
    """The built package of a checkout, beside any other checkout's already loaded (each keeps its own library)."""
    held = {k: sys.modules.pop(k) for k in list(sys.modules) if k == PKG_NAME or k.startswith(PKG_NAME + ".")}
    try:
        spec = importlib.util.spec_from_file_location("graft_entry_of_" + str(abs(hash(root))), os.path.join(root, "__graft_entry__.py"))
        g = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(g)
        pkg = g.load_package()
        pkg.load_library()
        return pkg
    finally:
        for k in [k for k in sys.modules if k == PKG_NAME or k.startswith(PKG_NAME + ".")]:
            del sys.modules[k]
        sys.modules.update(held)


class Hip:
    """the few HIP runtime calls the hand-written pattern needs, from the runtime the libraries are linked against"""

    def __init__(self, lib_path):
        L = C.CDLL(lib_path)
        vp = C.c_void_p
        for name, args in (("hipStreamCreateWithFlags", [C.POINTER(vp), C.c_uint]), ("hipStreamSynchronize", [vp]), ("hipStreamDestroy", [vp]),
                           ("hipEventCreateWithFlags", [C.POINTER(vp), C.c_uint]), ("hipEventRecord", [vp, vp]), ("hipEventDestroy", [vp]),
                           ("hipStreamWaitEvent", [vp, vp, C.c_uint]), ("hipMemcpyAsync", [vp, vp, C.c_size_t, C.c_int, vp]),
                           ("hipHostMalloc", [C.POINTER(vp), C.c_size_t, C.c_uint]), ("hipHostFree", [vp]),
                           ("hipMemGetInfo", [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, args
        self.L = L

    def ok(self, rc):
        assert rc == 0, f"HIP error {rc}"

    def stream(self):
        s = C.c_void_p()
        self.ok(self.L.hipStreamCreateWithFlags(C.byref(s), HIP_STREAM_NON_BLOCKING))
        return s.value

    def event(self):
        e = C.c_void_p()
        self.ok(self.L.hipEventCreateWithFlags(C.byref(e), HIP_EVENT_DISABLE_TIMING))
        return e.value

    def in_use(self):
        free, total = C.c_size_t(), C.c_size_t()
        self.ok(self.L.hipMemGetInfo(C.byref(free), C.byref(total)))
        return total.value - free.value


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


def unpack_rates(pkg, rows_out):
    """each unpack_* kernel on 2^26 sample frames, mono and stereo: bytes read + written per second (event times of the profile)"""
    n = 1 << 26
    with pkg.VoxBox(0) as vb:
        src = vb.empty(n * 2 * 8, np.uint8)
        vb._check(vb.L.vbx_memset(vb.ctx, src.ptr, 0x11, src.nbytes))
        out = vb.empty(n)
        for fmt, name, sb, ob in ((1, "unpack_pcm16", 2, 2), (2, "unpack_pcm24", 3, 8), (3, "unpack_pcm32", 4, 8), (4, "unpack_f32", 4, 4),
                                  (5, "unpack_f64", 8, 8)):
            for channels in (1, 2):
                vb.profile(True); vb.profile_reset()
                for _ in range(5):
                    vb.unpack_samples(src, n, fmt, channels, channels - 1, out=out)
                ms, cnt = vb.profile_report()[name]
                vb.profile(False)
                # interleaved channels share cache lines: the whole source is read
                nbytes = n * (sb * channels + ob)
                r = dict(case="unpack_kernel", kernel=name, channels=channels, sample_frames=n, bytes_per_launch=nbytes,
                         ms_per_launch=round(ms / cnt, 4), GBps=round(nbytes / (ms / cnt * 1e-3) / 1e9, 1),
                         fraction_of_hbm_roof=round(nbytes / (ms / cnt * 1e-3) / 1e9 / HBM_ROOF_GBPS, 3))
                print(json.dumps(r), flush=True)
                rows_out.append(r)


UNPACK_KERNELS = {1: "unpack_pcm16", 2: "unpack_pcm24", 3: "unpack_pcm32", 4: "unpack_f32", 5: "unpack_f64"}


def merge_trace(csv_path, rows):
    """adds trace_ns / trace_avg_ns / trace_GBps / trace_fraction_of_hbm_roof to the unpack rows from a rocprofv3 kernel trace of the
    --unpack run (one dispatch per launch: 2^26 sample frames are whole tiles of the tiled 24-bit kernel)"""
    import csv
    import re
    per = {}                                    # kernel name -> [ns per launch], in dispatch order
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            m = re.search(r"unpack_kernel<(\d)>", name)
            k = UNPACK_KERNELS[int(m.group(1))] if m else ("unpack_pcm24" if "unpack_pcm24_tiled_kernel" in name else None)
            if k is not None:
                per.setdefault(k, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for r in rows:
        if r.get("case") != "unpack_kernel":
            continue
        d = per[r["kernel"]]
        assert len(d) == 10, (r["kernel"], len(d))
        d = d[:5] if r["channels"] == 1 else d[5:]
        avg = statistics.mean(d)
        r.update(trace_ns=d, trace_avg_ns=round(avg), trace_GBps=round(r["bytes_per_launch"] / avg, 1),
                 trace_fraction_of_hbm_roof=round(r["bytes_per_launch"] / avg / HBM_ROOF_GBPS, 3),
                 source="trace_*: the rocprofv3 kernel trace of the --unpack run; ms_per_launch / GBps: the library profile's events in that run")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=HERE, help="the checkout whose built package runs (b) (default: this one)")
    ap.add_argument("--hours", type=float, default=4.0, help="length of the recording (at least 1)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--unpack", action="store_true", help="only the unpack_* kernels' rates (run this under rocprofv3 on its own)")
    ap.add_argument("--merge-trace", default=None, metavar="CSV", help="no GPU work: add the kernel trace's times to the unpack rows of --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows, kept = [], []
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            kept = json.load(f)
    if args.merge_trace:
        assert args.out and kept, "--merge-trace works on the report --out names"
        merge_trace(args.merge_trace, kept)
        rows, kept = kept, []
    elif args.unpack:
        kept = [r for r in kept if r.get("case") != "unpack_kernel"]
        unpack_rates(load_package(HERE), rows)
    else:
        kept = [r for r in kept if r.get("case") == "unpack_kernel"]
        pkg = load_package(HERE)
        assert args.runs >= 3 and args.hours >= 1.0
        root_b = os.path.abspath(args.root)
        pkg_p = pkg if root_b == HERE else load_package(root_b)
        bench(args, pkg, pkg_p, root_b, rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump((rows + kept) if not args.unpack else (kept + rows), f, indent=1)
            f.write("\n")


def bench(args, pkg, pkg_p, root_b, rows):
    def emit(**r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    CH = pkg.HOST_DEFAULT_CHUNK_FRAMES
    assert CH % SEG_FRAMES == 0
    F = int(round(args.hours * 3600 * SR / H)); F -= F % CH; F = max(F, CH)      # whole chunks: the only form the pattern handles
    n_chunks = F // CH
    ns, ns_chunk = (F - 1) * H + N, (CH - 1) * H + N
    hip = Hip(pkg.LIB_PATH)
    main_p = hip.stream()
    with pkg.VoxBox(0) as va, pkg_p.VoxBox(0, main_p) as vp:
        name, _ = va.device_info()
        common = dict(frames=F, hours=round(F * H / SR / 3600, 3), frame_len=N, stride=H, chunk_frames=CH, device=name,
                      root=os.path.basename(HERE), root_parent=os.path.basename(root_b))
        est = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
        params = pkg.AnalysisParams.make(SR, formant_order=ORDER, est_init=est)
        params_p = pkg_p.AnalysisParams.make(SR, formant_order=ORDER, est_init=est)
        rec = int(va.L.vbx_record_doubles(params)); rec += rec & 1
        # the recording: synthetic speech quantised to int16 (as bench_host_fed builds it), in pinned host memory
        host = va.malloc_host(ns, np.int16)
        for c in range(n_chunks):
            d = va.synth_speech(ns_chunk, sample_offset=c * CH * H, sample_rate=SR)
            host[c * CH * H:c * CH * H + ns_chunk] = np.clip(np.round(d.numpy() * (0.9 * 32767.0 / 0.5)), -32768, 32767).astype(np.int16)
            d.free()
        used0 = hip.in_use()
        seg_all = np.arange(0, F, SEG_FRAMES, dtype=np.int64)
        out_a, st_a = va.empty((F, rec)), va.empty((3, F), np.int32)

        def host_call(seg=seg_all):
            va.analyze_host(host, params, seg_start=seg, frame_len=N, stride=H, out=out_a, record_ld=rec, status=st_a)
            va.sync()

        host_call()
        used_a = hip.in_use()

        # (b): the documented pattern on the parent build
        out_p, st_p = vp.empty((F, rec)), vp.empty((3, CH), np.int32)
        bufs = [vp.empty(ns_chunk, np.int16) for _ in range(2)]
        copy = hip.stream()
        ready, freed = [hip.event() for _ in range(2)], [hip.event() for _ in range(2)]
        seg_chunk = np.arange(0, CH, SEG_FRAMES, dtype=np.int64)
        base = host.ctypes.data

        def upload(c):
            b = c % 2
            hip.ok(hip.L.hipStreamWaitEvent(copy, freed[b], 0))
            hip.ok(hip.L.hipMemcpyAsync(bufs[b].ptr, base + 2 * c * CH * H, 2 * ns_chunk, HIP_MEMCPY_H2D, copy))
            hip.ok(hip.L.hipEventRecord(ready[b], copy))

        def pattern_parent():
            for b in range(2):
                hip.ok(hip.L.hipEventRecord(freed[b], main_p))
            upload(0)
            for c in range(n_chunks):
                b = c % 2
                if c + 1 < n_chunks:
                    upload(c + 1)
                hip.ok(hip.L.hipStreamWaitEvent(main_p, ready[b], 0))
                vp.analyze_frames_pcm16(bufs[b].ptr, params_p, seg_start=seg_chunk, frame_len=N, stride=H, n_frames=CH,
                                        out=out_p.ptr + 8 * c * CH * rec, record_ld=rec, status=st_p)
                hip.ok(hip.L.hipEventRecord(freed[b], main_p))
            vp.sync()
            hip.ok(hip.L.hipStreamSynchronize(copy))

        def host_call_one():
            host_call(None)

        # (d): the recording resident
        pattern_parent()
        used_c = hip.in_use()
        x_res = va.to_device(host, np.int16)

        def resident():
            va.analyze_frames_ex_pcm16(x_res, params, None, None, seg_start=seg_all, frame_len=N, stride=H, n_frames=F, out=out_a, record_ld=rec,
                                       status=st_a)
            va.sync()

        resident()
        used_d = hip.in_use()
        # the host call: everything allocated since the recording was built (records, status rows, the slots, the chunk-sized workspaces);
        # the resident call: the same outputs plus what appeared when the recording was uploaded and analysed whole
        emit(case="device_bytes", recording=2 * ns, records=8 * F * rec, status3=12 * F, in_use_host_call=used_a - used0,
             in_use_resident_call=8 * F * rec + 12 * F + (used_d - used_c), **common)
        cases = [("host_call", host_call), ("pattern_parent", pattern_parent), ("host_call_one", host_call_one), ("resident_pcm16", resident)]
        ms = alternate([fn for _, fn in cases], args.warmup, args.runs)
        med = {}
        for (case, _), t in zip(cases, ms):
            med[case] = statistics.median(t)
            emit(case=case, ms=round(med[case], 3), all_ms=[round(x, 3) for x in t], spread_ms=round(max(t) - min(t), 3),
                 frames_per_s=F / (med[case] * 1e-3), **common)
        spread = max(max(t) - min(t) for (case, _), t in zip(cases, ms) if case in ("host_call", "pattern_parent"))
        emit(case="bar", host_call_ms=round(med["host_call"], 3), pattern_parent_ms=round(med["pattern_parent"], 3), allowed_ms=round(spread, 3),
             met=bool(med["host_call"] <= med["pattern_parent"] + spread),
             host_call_over_resident=round(med["resident_pcm16"] / med["host_call"], 4),
             host_call_one_over_resident=round(med["resident_pcm16"] / med["host_call_one"], 4), **common)
        # the same bits: the host call's records against the resident call's, the first and the last frames
        resident()
        k = min(F, 200_000) * rec
        want = [out_a.numpy_slice(s, k).view(np.int64) for s in (0, F * rec - k)]
        host_call()
        same = all(np.array_equal(out_a.numpy_slice(s, k).view(np.int64), w) for s, w in zip((0, F * rec - k), want))
        emit(case="host_call_bits_equal_resident", equal=bool(same), frames_compared=2 * min(F, 200_000), **common)
        va.free_host(host)
    hip.ok(hip.L.hipStreamSynchronize(copy))
    hip.ok(hip.L.hipStreamDestroy(copy))
    hip.ok(hip.L.hipStreamDestroy(main_p))


if __name__ == "__main__":
    main()
