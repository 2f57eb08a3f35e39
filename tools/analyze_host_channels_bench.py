#!/usr/bin/env python3
"""Times vbx_analyze_host_channels -- every channel of a host-resident recording from ONE upload per chunk -- against what a caller
had to write before it: one vbx_analyze_host call per channel on the build under --root (the PARENT commit's), each uploading the
interleaved frames again.  The bench's 1200 / 480 pipeline (48 kHz, every part on) over interleaved 16-bit PCM in pinned host memory,
at the default chunk_frames, on one MI355X.  The cases ALTERNATE in one process, median of --runs after a warm-up, each case closed by
a synchronise and timed on the host clock (the uploads are part of what is measured).  Per channel count C in --channels:

  parent_calls_C     C successive vbx_analyze_host calls on the parent build, no wait between them, one synchronise at the end;
  channels_call_C    ONE vbx_analyze_host_channels call on this build, every channel selected.

The bar, per C: the new median is not above the parent pattern's by more than the larger of the two cases' spreads.  Also reported:
the speed-up, the device memory in use (hipMemGetInfo) with the new call's buffers, the per-kernel times of one profiled run of the
new call (where the time goes), and the first and last 200,000 frames of every channel's records against the parent pattern's, bit
for bit.

--unpack (meant to be run on its own under `rocprofv3 --kernel-trace --stats`, never together with --pmc): one unpack_all_* launch
producing all C planes against the SUM of the C per-channel unpack_* launches of the parent build, per format, at 2^26 sample frames
for 2 channels and 2^24 for 8 (planes n + 128 elements apart: 256-byte aligned, not a power of two apart); bytes moved per second and
the fraction of the HBM roof, from the libraries' profile events.  Rows with "selected": 1 are the same launch with ONE channel selected
(the LDS gather's worst case) against the parent's one launch for that channel.

--out FILE keeps the rows of the OTHER mode that FILE already holds, so the two steps build one report:

  python tools/analyze_host_channels_bench.py --root ../parent_checkout --out profiles/analyze_host_channels/report.json
  rocprofv3 --kernel-trace --stats -d DIR -o unpack --output-format csv -- \\
      python tools/analyze_host_channels_bench.py --root ../parent_checkout --unpack --out profiles/analyze_host_channels/report.json"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from analyze_host_bench import HBM_ROOF_GBPS, HERE, Hip, H, N, ORDER, SR, alternate, load_package  # noqa: E402

FORMATS = ((1, "pcm16", 2, 2), (2, "pcm24", 3, 8), (3, "pcm32", 4, 8), (4, "f32", 4, 4), (5, "f64", 8, 8))


def unpack_rates(pkg, pkg_p, rows_out):
    """one unpack_all launch for all planes against the parent's C single-channel launches (the profile's event times, 5 launches)"""
    with pkg.VoxBox(0) as va, pkg_p.VoxBox(0) as vp:
        for channels, n in ((2, 1 << 26), (8, 1 << 24)):
            src = va.empty(n * channels * 8, np.uint8)
            va._check(va.L.vbx_memset(va.ctx, src.ptr, 0x11, src.nbytes))
            ld = n + 128                                            # planes 256-byte aligned and NOT a power of two apart, as the host call lays them out
            out = va.empty((channels, ld))
            va.sync()
            for fmt, tag, sb, ob in FORMATS:
                va.profile(True); va.profile_reset()
                for _ in range(5):
                    va.unpack_channels(src, n, fmt, channels, out=out, plane_ld=ld)
                ms, cnt = va.profile_report()["unpack_all_" + tag]
                va.profile(False)
                new_ms = ms / cnt
                vp.profile(True); vp.profile_reset()
                for _ in range(5):
                    for c in range(channels):
                        vp.unpack_samples(src.ptr, n, fmt, channels, c, out=out.ptr)
                ms, cnt = vp.profile_report()["unpack_" + tag]
                vp.profile(False)
                parent_ms = ms / cnt * channels                     # the C launches that produce the same planes
                nbytes = n * channels * (sb + ob)                   # every source byte read once, every plane written
                r = dict(case="unpack_all_kernel", kernel="unpack_all_" + tag, channels=channels, sample_frames=n, plane_ld=ld, bytes_per_launch=nbytes,
                         ms_per_launch=round(new_ms, 4), GBps=round(nbytes / (new_ms * 1e-3) / 1e9, 1),
                         fraction_of_hbm_roof=round(nbytes / (new_ms * 1e-3) / 1e9 / HBM_ROOF_GBPS, 3),
                         parent_launches=channels, parent_sum_ms=round(parent_ms, 4), speedup=round(parent_ms / new_ms, 3),
                         met=bool(new_ms <= parent_ms))
                print(json.dumps(r), flush=True)
                rows_out.append(r)
                # ONE channel selected: the fewest planes for the lanes to spread over (the LDS gather's worst case), against the
                # parent's one launch for that channel
                va.profile(True); va.profile_reset()
                for _ in range(5):
                    va.unpack_channels(src, n, fmt, channels, select=[channels - 1], out=out, plane_ld=ld)
                ms, cnt = va.profile_report()["unpack_all_" + tag]
                va.profile(False)
                one_ms, nb1 = ms / cnt, n * (channels * sb + ob)
                r = dict(case="unpack_all_kernel", kernel="unpack_all_" + tag, channels=channels, selected=1, sample_frames=n, plane_ld=ld,
                         bytes_per_launch=nb1, ms_per_launch=round(one_ms, 4), GBps=round(nb1 / (one_ms * 1e-3) / 1e9, 1),
                         fraction_of_hbm_roof=round(nb1 / (one_ms * 1e-3) / 1e9 / HBM_ROOF_GBPS, 3), parent_launches=1,
                         parent_sum_ms=round(parent_ms / channels, 4), speedup=round(parent_ms / channels / one_ms, 3),
                         met=bool(one_ms <= parent_ms / channels))
                print(json.dumps(r), flush=True)
                rows_out.append(r)
            va.sync(); vp.sync()
            src.free(); out.free()


def bench(args, pkg, pkg_p, root_b, rows):
    def emit(**r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    CH = pkg.HOST_DEFAULT_CHUNK_FRAMES
    F = max(int(round(args.hours * 3600 * SR / H)), 1)
    ns = (F - 1) * H + N
    hip = Hip(pkg.LIB_PATH)
    counts = [int(c) for c in args.channels.split(",")]
    cmax = max(counts)
    with pkg.VoxBox(0) as va, pkg_p.VoxBox(0) as vp:
        name, _ = va.device_info()
        common = dict(frames=F, hours=round(F * H / SR / 3600, 3), frame_len=N, stride=H, chunk_frames=CH, chunks=-(-F // CH), device=name,
                      root=os.path.basename(HERE), root_parent=os.path.basename(root_b))
        est = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
        params = pkg.AnalysisParams.make(SR, formant_order=ORDER, est_init=est)
        params_p = pkg_p.AnalysisParams.make(SR, formant_order=ORDER, est_init=est)
        rec = int(va.L.vbx_record_doubles(params)); rec += rec & 1
        # one channel of synthetic speech quantised to int16; the others are that channel rolled and, every other one, negated
        mono = np.empty(ns, np.int16)
        step = 1 << 24
        for s in range(0, ns, step):
            m = min(step, ns - s)
            d = va.synth_speech(m, sample_offset=s, sample_rate=SR)
            mono[s:s + m] = np.clip(np.round(d.numpy() * (0.9 * 32767.0 / 0.5)), -32767, 32767).astype(np.int16)
            d.free()
        outs_a = [(va.empty((F, rec)), va.empty((3, F), np.int32)) for _ in range(cmax)]
        outs_p = [(vp.empty((F, rec)), vp.empty((3, F), np.int32)) for _ in range(cmax)]
        for C in counts:
            host = va.malloc_host((ns, C), np.int16)
            for j in range(C):
                host[:, j] = np.roll(mono, 7919 * j) * (-1 if j & 1 else 1)
            used0 = hip.in_use()

            def channels_call():
                va.analyze_host_channels(host, params, frame_len=N, stride=H, out=[o[0] for o in outs_a[:C]], record_ld=rec,
                                         status=[o[1] for o in outs_a[:C]])
                va.sync()

            def parent_calls():
                for c in range(C):
                    vp.analyze_host(host, params_p, channel=c, frame_len=N, stride=H, out=outs_p[c][0], record_ld=rec, status=outs_p[c][1])
                vp.sync()

            channels_call()
            used_a = hip.in_use()
            parent_calls()
            used_p = hip.in_use()
            emit(case="device_bytes", channels=C, recording=2 * ns * C, records=8 * F * rec * C, status3=12 * F * C,
                 in_use_channels_call=used_a - used0, in_use_parent_calls_on_top=used_p - used_a, **common)
            cases = [(f"channels_call_{C}", channels_call), (f"parent_calls_{C}", parent_calls)]
            ms = alternate([fn for _, fn in cases], args.warmup, args.runs)
            med = {}
            for (case, _), t in zip(cases, ms):
                med[case] = statistics.median(t)
                emit(case=case, channels=C, ms=round(med[case], 3), all_ms=[round(x, 3) for x in t], spread_ms=round(max(t) - min(t), 3),
                     channel_frames_per_s=C * F / (med[case] * 1e-3), uploaded_bytes=2 * ns * C * (1 if case.startswith("channels") else C),
                     **common)
            spread = max(max(t) - min(t) for t in ms)
            new, old = med[f"channels_call_{C}"], med[f"parent_calls_{C}"]
            emit(case="bar", channels=C, channels_call_ms=round(new, 3), parent_calls_ms=round(old, 3), allowed_ms=round(spread, 3),
                 met=bool(new <= old + spread), speedup=round(old / new, 3), **common)
            # where the new call's time goes: the per-kernel event times of one profiled run
            va.profile(True); va.profile_reset()
            channels_call()
            rep = va.profile_report()
            va.profile(False)
            emit(case="profile", channels=C, kernels_ms={k: [round(v[0], 3), int(v[1])] for k, v in sorted(rep.items())}, **common)
            # the same bits: the first and the last 200,000 frames of every channel
            channels_call()
            parent_calls()
            k = min(F, 200_000) * rec
            same = all(np.array_equal(outs_a[c][0].numpy_slice(s, k).view(np.int64), outs_p[c][0].numpy_slice(s, k).view(np.int64))
                       for c in range(C) for s in (0, F * rec - k))
            emit(case="bits_equal_parent_calls", channels=C, equal=bool(same), frames_compared_per_channel=2 * min(F, 200_000), **common)
            va.sync(); vp.sync()
            va.free_host(host)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=HERE, help="the checkout whose built package runs the parent pattern (default: this one)")
    ap.add_argument("--hours", type=float, default=1.0, help="length of the recording (an hour of 8 channels is 2.8 GB of pinned memory)")
    ap.add_argument("--channels", default="2,8")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--unpack", action="store_true", help="only the unpack kernels' rates (run this under rocprofv3 on its own)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows, kept = [], []
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            kept = json.load(f)
    pkg = load_package(HERE)
    root_b = os.path.abspath(args.root)
    pkg_p = pkg if root_b == HERE else load_package(root_b)
    if args.unpack:
        kept = [r for r in kept if r.get("case") != "unpack_all_kernel"]
        unpack_rates(pkg, pkg_p, rows)
    else:
        kept = [r for r in kept if r.get("case") == "unpack_all_kernel"]
        assert args.runs >= 3
        bench(args, pkg, pkg_p, root_b, rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump((rows + kept) if not args.unpack else (kept + rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
