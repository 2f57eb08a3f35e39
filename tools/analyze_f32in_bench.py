#!/usr/bin/env python3
"""Times the fused frame loop on float32 samples against what a float caller had before it, on the bench's utterance (1200 / 480 at
48 kHz, 4.5 M frames, every part on), with HIP events on the context's stream, the cases ALTERNATING in one process after a warm-up:

  (a0) f64_parent   vbx_analyze_frames_ex_f64 on the f64 samples, from the build under --root (the PARENT commit's: the yardstick);
  (a)  f64          the same call from THIS checkout;
  (b)  widen_f64    vbx_f32_to_f64 into a caller-owned buffer, then (a): what a caller holding a float32 tensor does without the
                    new entry point -- an extra pass, and 4 + 8 bytes per sample resident;
  (c)  f32in        vbx_analyze_frames_ex_f32in on the float samples.

The f64 samples ARE the exactly widened float samples, so the three forms compute the same records (a slice of them is compared bit
for bit).  Device memory in use (hipMemGetInfo) is read before anything is allocated, after (c) has run with only the float samples
resident, and after (b) has run with the widened copy beside them.  --frame-len 1024 --stride 512 measures a widened-first shape:
there (c) runs the widening pass itself, into a context-owned copy.  One JSON line per row; --out FILE writes the list of them.

  python tools/analyze_f32in_bench.py --root ../parent_checkout --out profiles/analyze_f32in/report.json"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, ORDER = 48000.0, 12
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
    vb.profile(False)
    return rep


_hip = None


def device_bytes_in_use():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert _hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=HERE, help="the checkout whose built package runs (a0) (default: this one)")
    ap.add_argument("--frames", type=int, default=4_500_000)
    ap.add_argument("--frame-len", type=int, default=1200)
    ap.add_argument("--stride", type=int, default=480)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.runs >= 3
    N, H, F = args.frame_len, args.stride, args.frames
    root_b = os.path.abspath(args.root)
    pkg = load_package(HERE)
    pkg_p = pkg if root_b == HERE else load_package(root_b)
    rows = []

    def emit(**r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    ns = (F - 1) * H + N
    with pkg.VoxBox(0) as va, pkg_p.VoxBox(0) as vp:
        name, _ = va.device_info()
        path = "native" if N == 1200 else "widened_first"
        common = dict(frames=F, frame_len=N, stride=H, path=path, device=name, root=os.path.basename(HERE), root_parent=os.path.basename(root_b))
        est = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
        params = pkg.AnalysisParams.make(SR, formant_order=ORDER, est_init=est)
        params_p = pkg_p.AnalysisParams.make(SR, formant_order=ORDER, est_init=est)
        rec = int(va.L.vbx_record_doubles_ex(params, None)); rec += rec & 1
        used0 = device_bytes_in_use()
        # the float samples: a synthetic piece, rounded to float32 on the host and tiled over the recording
        piece_n = min(45_000 * H, ns)
        d = va.synth_speech(piece_n, sample_offset=0, sample_rate=SR)
        piece = d.numpy().astype(np.float32)
        d.free()
        x32 = va.empty(ns, np.float32)
        for off in range(0, ns, piece.size):
            n = min(piece.size, ns - off)
            va._check(va.L.vbx_memcpy_h2d(va.ctx, x32.ptr + 4 * off, piece.ctypes.data, 4 * n))
        out_c, st_c = va.empty((F, rec)), va.empty((3, F), np.int32)

        def f32in():
            va.analyze_frames_ex_f32in(x32, params, None, None, frame_len=N, stride=H, n_frames=F, out=out_c, record_ld=rec, status=st_c)

        f32in(); va.sync()
        used_c = device_bytes_in_use()
        x64 = va.empty(ns)

        def f64():
            va.analyze_frames_ex(x64, params, None, None, frame_len=N, stride=H, n_frames=F, out=out_c, record_ld=rec, status=st_c)

        def widen_f64():
            va._check(va.L.vbx_f32_to_f64(va.ctx, x32.ptr, ns, x64.ptr))
            f64()

        widen_f64(); va.sync()
        used_b = device_bytes_in_use()
        emit(case="device_bytes", samples_f32=4 * ns, samples_f64=8 * ns, records=8 * F * rec, status3=12 * F,
             in_use_after_f32in=used_c - used0, in_use_after_widen_f64=used_b - used0, **common)
        out_p, st_p = vp.empty((F, rec)), vp.empty((3, F), np.int32)

        def f64_parent():
            vp.analyze_frames_ex(x64.ptr, params_p, None, None, frame_len=N, stride=H, n_frames=F, out=out_p, record_ld=rec, status=st_p)

        cases = [("f64_parent", vp, f64_parent), ("f64", va, f64), ("widen_f64", va, widen_f64), ("f32in", va, f32in)]
        ms = alternate([(v, fn) for _, v, fn in cases], args.warmup, args.runs)
        for (case, v, fn), t in zip(cases, ms):
            med = statistics.median(t)
            emit(case=case, ms=round(med, 3), all_ms=[round(x, 3) for x in t], spread_ms=round(max(t) - min(t), 3),
                 frames_per_s=F / (med * 1e-3), **common)
        for case, v, fn in cases[1:]:
            emit(case=case + "_kernels", kernels_ms=kernels(v, fn), **common)
        # the same bits: the float call's records against the parent's f64 call's, the first and the last frames
        f32in(); va.sync()
        k = min(F, 200_000) * rec
        same = all(np.array_equal(out_c.numpy_slice(s, k).view(np.int64), out_p.numpy_slice(s, k).view(np.int64)) for s in (0, F * rec - k))
        emit(case="f32in_bits_equal_parent_f64", equal=bool(same), frames_compared=2 * min(F, 200_000), **common)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
