#!/usr/bin/env python3
"""Times the formant_extraction example's frame loop from ONE call against the sequence of calls it replaces, on the bench's
utterance (1200 / 480 at 48 kHz, 4.5 M frames = 12.5 h, every part on, formants at ratio 10000 / 48000 and order 12, RMS on), with
HIP events on the context's stream, median of --runs calls after a warm-up:

  (a) ex         vbx_analyze_frames_ex_f64, and vbx_analyze_frames_ex_pcm16 on 16-bit PCM -- from THIS checkout;
  (b) sequence   what a caller needs without it: vbx_analyze_frames_f64 with formant_order = 0, vbx_resample_linear_f64 into a
                 caller-owned dense [F, m] batch, vbx_find_formants_f64 on it, vbx_rms_f64; on PCM vbx_pcm16_to_f64 into a
                 caller-owned copy first.  It uses nothing this entry point added, so it runs from an older checkout:
                 --root DIR loads that tree's built package -- the baseline is the sequence built from the PARENT commit.

(a) and (b) ALTERNATE inside one process (one context per build, the same device buffers), so both see the same clocks.  Each
case is followed by its per-kernel event times (vbx_profile_*; kernels on the side stream overlap the context stream's), and
the caller-side and context-side bytes of both forms are reported.  --m 250 300 also times the formant chain alone
(vbx_find_formants_resampled_f64 against resample + vbx_find_formants_f64) at those resampled lengths: the loader's own cost.
One JSON line per row; --out FILE writes the list of all of them.

  python tools/analyze_example_bench.py --root ../parent_checkout --out profiles/analyze_example/report.json"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, SR, ORDER = 1200, 480, 48000.0, 12
PKG_NAME = "vox_box_rs_amd"


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


def alternate(cases, warmup, runs):
    """cases: [(vb, fn)].  Every case once per round, in order; returns the per-case lists of event times (ms)."""
    for _ in range(warmup):
        for vb, fn in cases:
            fn()
            vb.sync()
    ms = [[] for _ in cases]
    for _ in range(runs):
        for i, (vb, fn) in enumerate(cases):
            vb.timer_begin()
            fn()
            ms[i].append(vb.timer_end())
    return ms


def kernels(vb, fn):
    vb.profile(True); vb.profile_reset(); fn()
    rep = {k: round(v[0], 3) for k, v in vb.profile_report().items()}
    streams = vb.profile_streams() if hasattr(vb, "profile_streams") else {}
    vb.profile(False)
    return rep, streams


def make_pcm(vb, audio_piece, ns):
    s = np.clip(np.rint(audio_piece * 20000.0), -32768, 32767).astype(np.int16)
    pcm = vb.empty(ns, np.int16)
    for off in range(0, ns, s.size):
        n = min(s.size, ns - off)
        vb._check(vb.L.vbx_memcpy_h2d(vb.ctx, pcm.ptr + 2 * off, s.ctypes.data, 2 * n))
    return pcm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=HERE, help="the checkout whose built package runs the sequence (default: this one)")
    ap.add_argument("--frames", type=int, default=4_500_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ratio", type=float, default=10000.0 / 48000.0)
    ap.add_argument("--m", type=int, nargs="*", default=[], help="also time the formant chain alone at these resampled lengths (ratio = m / 1200)")
    ap.add_argument("--no-pcm", action="store_true")
    ap.add_argument("--chain-only", action="store_true", help="only the --m cases (a kernel-trace run of the loaders)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 1
    root_b = os.path.abspath(args.root)
    pkg_a = load_package(HERE)
    pkg_b = pkg_a if root_b == HERE else load_package(root_b)
    rows = []

    def emit(**r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    F = args.frames
    ns = (F - 1) * H + N
    with pkg_a.VoxBox(0) as va, pkg_b.VoxBox(0) as vb:
        name, _ = va.device_info()
        common = dict(frames=F, frame_len=N, stride=H, order=ORDER, device=name, root_a=os.path.basename(HERE), root_b=os.path.basename(root_b))
        audio = va.synth_speech(ns, sample_offset=0, sample_rate=SR)             # device memory: both contexts read it
        est = np.array([[f, 1.0] for f in pkg_a.MALE_FORMANT_ESTIMATES])
        params_a = pkg_a.AnalysisParams.make(SR, formant_order=ORDER, est_init=est)
        rest_b = pkg_b.AnalysisParams.make(SR, formant_order=0)
        ext = pkg_a.AnalysisExt.make(args.ratio, rms=True)
        m = int(va.L.vbx_resampled_len(N, args.ratio))
        rate = SR * args.ratio
        rec_a = int(va.L.vbx_record_doubles_ex(params_a, ext)); rec_a += rec_a & 1
        rec_b = int(vb.L.vbx_record_doubles(rest_b)); rec_b += rec_b & 1
        out_a, st_a = va.empty((F, rec_a)), va.empty((3, F), np.int32)
        out_b, st_b = vb.empty((F, rec_b)), vb.empty((3, F), np.int32)
        dense, form_b, fst_b, rms_b = vb.empty((F, m)), vb.empty((F, 4, 2)), vb.empty(F, np.int32), vb.empty(F)
        bufs_b = {"formants": form_b, "status": fst_b}
        piece = min(450_000 * H, ns)
        pcm = None if args.no_pcm or args.chain_only else make_pcm(va, audio.numpy_slice(0, piece), ns)
        wide = None if pcm is None else vb.empty(ns)

        def ex_f64():
            va.analyze_frames_ex(audio, params_a, ext, None, frame_len=N, stride=H, n_frames=F, out=out_a, record_ld=rec_a, status=st_a)

        def ex_pcm():
            va.analyze_frames_ex_pcm16(pcm, params_a, ext, None, frame_len=N, stride=H, n_frames=F, out=out_a, record_ld=rec_a, status=st_a)

        def seq(x):
            vb.analyze_frames(x, rest_b, frame_len=N, stride=H, n_frames=F, out=out_b, record_ld=rec_b, status=st_b)
            vb.resample_linear(x, args.ratio, frame_len=N, stride=H, n_frames=F, out=dense)
            vb.find_formants(dense, rate, ORDER, est, frame_len=m, stride=m, n_frames=F, out=bufs_b)
            vb._check(vb.L.vbx_rms_f64(vb.ctx, x, F, N, H, None, rms_b.ptr))

        def seq_f64():
            seq(audio.ptr)                                                       # (a raw pointer: the buffer is the other package's)

        def seq_pcm():
            vb._check(vb.L.vbx_pcm16_to_f64(vb.ctx, pcm.ptr, ns, wide.ptr))
            seq(wide.ptr)

        pairs = [("f64", ex_f64, seq_f64)] + ([] if pcm is None else [("pcm16", ex_pcm, seq_pcm)])
        if args.chain_only:
            pairs = []
        for label, fa, fb in pairs:
            ms_a, ms_b = alternate([(va, fa), (vb, fb)], args.warmup, args.runs)
            for case, ms in (("ex_" + label, ms_a), ("sequence_" + label, ms_b)):
                med = statistics.median(ms)
                emit(case=case, ms=round(med, 3), all_ms=[round(v, 3) for v in ms], spread_ms=round(max(ms) - min(ms), 3),
                     frames_per_s=F / (med * 1e-3), **common)
            for case, v, fn in (("ex_" + label, va, fa), ("sequence_" + label, vb, fb)):
                rep, streams = kernels(v, fn)
                emit(case=case + "_kernels", kernels_ms=rep, streams=streams)
        # bytes: what the caller must own, and what the context holds for the call
        caller_a = dict(samples_f64=8 * ns, samples_pcm16=2 * ns, records=8 * F * rec_a, status3=12 * F)
        caller_b = dict(samples_f64=8 * ns, samples_pcm16=2 * ns, widened_copy_for_pcm=8 * ns, records=8 * F * rec_b, status3=12 * F,
                        dense_batch=8 * F * m, formants=64 * F, formant_status=4 * F, rms=8 * F)
        # context-side: the formant chain's workspaces (Burg coefficients, resonance rows, counts) are the same in both forms; only
        # a shape without a PCM kernel adds the context-owned widened copy (not this one: 1200-sample frames read the PCM directly)
        chain = F * (8 * ORDER + 16 * 32 + 4)
        if not args.chain_only:
            emit(case="bytes", caller_ex=caller_a, caller_sequence=caller_b, m=m, context_formant_chain_either_form=chain)

        # the formant chain alone at other resampled lengths: the loader against the dense batch
        for mm in args.m:
            r = mm / N
            assert int(va.L.vbx_resampled_len(N, r)) == mm
            d2 = vb.empty((F, mm))
            form_a, fst_a = va.empty((F, 4, 2)), va.empty(F, np.int32)
            bufs_a = {"formants": form_a, "status": fst_a}

            def chain_a():
                va.find_formants(audio, SR * r, ORDER, est, frame_len=N, stride=H, n_frames=F, out=bufs_a, resample_ratio=r)

            def chain_b():
                vb.resample_linear(audio.ptr, r, frame_len=N, stride=H, n_frames=F, out=d2)
                vb.find_formants(d2, SR * r, ORDER, est, frame_len=mm, stride=mm, n_frames=F, out=bufs_b)
            ms_a, ms_b = alternate([(va, chain_a), (vb, chain_b)], args.warmup, args.runs)
            for case, ms, v, fn in (("chain_resampled", ms_a, va, chain_a), ("chain_dense", ms_b, vb, chain_b)):
                rep, _ = kernels(v, fn)
                emit(case=case, m=mm, ms=round(statistics.median(ms), 3), all_ms=[round(x, 3) for x in ms], kernels_ms=rep)
            same = np.array_equal(form_a.numpy().view(np.int64), form_b.numpy().view(np.int64)) and np.array_equal(fst_a.numpy(), fst_b.numpy())
            emit(case="chain_bits_equal", m=mm, equal=bool(same))
            for d in (d2, form_a, fst_a):
                d.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
