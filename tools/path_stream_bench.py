#!/usr/bin/env python3
"""Times the online pitch path (vbx_path_stream_*, vbx_session_path_bind) on one MI355X.  All round trips are a host clock around
a call that ENDS IN vbx_sync; the two sides of every comparison alternate in one process after a warm-up, and the spread of the
repeats is reported with each median.  The lists are those of the bench's synthetic speech (1200 / 480 at 48 kHz).

  push     a push round trip at 1 / 10 / 100 frames per push, kmax 4 and 15, against the only exact incremental form a caller had
           before: vbx_pitch_path_f64 rerun over the utterance so far after every push (hand-written here against the same library).
           Both must write the same bits on the rows the online path has committed.
  large    the kernel's own time per frame on ONE large push (the library's event profile), beside the resident call's sequential
           form (chunk_frames = n_frames) and its chunked default on the same lists.
  session  a bound session's 1-hop push against the same session unbound, alternating in one run.
  delay    the commit delay in frames, frame by frame, on the three golden recordings.
  --trace  only a warmed run of --pushes 1-hop pushes of a BOUND session, meant to run on its own under
           `rocprofv3 --kernel-trace --stats`; --count-trace CSV then counts the dispatches per push in that trace (no GPU work).

  python tools/path_stream_bench.py --out profiles/path_stream/report.json"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import statistics
import sys
import time
import wave

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SR, N, H, MP = 48000.0, 1200, 480, 64


def emit(rows, **r):
    print(json.dumps(r), flush=True)
    rows.append(r)


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "runs": len(v)}


def speech_lists(pkg, vb, F, kmax, x=None, sr=SR, n=N, h=H):
    """device lists (cand, count, status, peak) of F frames"""
    xd = vb.synth_speech((F - 1) * h + n, sample_offset=5 * 48000 + 321) if x is None else vb.to_device(x)
    cand, cnt, st, pk = vb.empty((F, kmax, 2)), vb.empty(F, np.int32), vb.empty(F, np.int32), vb.empty(F)
    vb.pitch(xd, sr, 0.2, 75.0, 600.0, kmax=kmax, frame_len=n, stride=h, n_frames=F, window=vb.window(pkg.WINDOW_HANNING, n), out=(cand, cnt, st))
    vb.frame_peak(xd, frame_len=n, stride=h, n_frames=F, out=pk)
    vb.sync()
    xd.free()
    return cand, cnt, st, pk


def push_case(pkg, vb, rows, args):
    for kmax in (4, 15):
        for fpp in (1, 10, 100):
            pushes = args.pushes
            F = fpp * pushes
            cand, cnt, st, pk = speech_lists(pkg, vb, F, kmax)
            par = pkg.PitchPathParams.make(time_step=H / SR, silence_threshold=0.0)
            rpp = MP + fpp
            path, idx, forced, com = vb.empty((pushes * rpp, 2)), vb.empty(pushes * rpp, np.int32), vb.empty(pushes * rpp, np.uint8), vb.empty((pushes, 4), np.int64)
            path_b, idx_b = vb.empty((F, 2)), vb.empty(F, np.int32)
            ps = vb.path_stream(kmax, par, max_pending=MP)

            def run_online(times):
                ps.reset()
                for i in range(pushes):
                    t = i * fpp
                    t0 = time.perf_counter()
                    ps.push(cand.ptr + t * kmax * 16, cnt.ptr + 4 * t, st.ptr + 4 * t, None, n_frames=fpp,
                            out=(path.ptr + 16 * i * rpp, idx.ptr + 4 * i * rpp, forced.ptr + i * rpp, com.ptr + 32 * i))
                    vb.sync()
                    times.append((time.perf_counter() - t0) * 1e3)

            def run_rerun(times):
                for i in range(pushes):
                    t0 = time.perf_counter()
                    vb.pitch_path(cand, cnt, st, None, params=par, n_frames=(i + 1) * fpp, kmax=kmax, out=(path_b, idx_b))
                    vb.sync()
                    times.append((time.perf_counter() - t0) * 1e3)
            per = {"online": [], "rerun": []}
            for r in range(args.warmup + args.runs):
                for k, fn in (("online", run_online), ("rerun", run_rerun)):
                    t = []
                    fn(t)
                    if r >= args.warmup:
                        per[k].append(statistics.median(t))
            cm, p, ix, fo = com.numpy(), path.numpy(), idx.numpy(), forced.numpy()
            got_p = np.concatenate([p[i * rpp:i * rpp + cm[i, 1]] for i in range(pushes)])
            got_i = np.concatenate([ix[i * rpp:i * rpp + cm[i, 1]] for i in range(pushes)])
            k = got_p.shape[0]
            ok = np.concatenate([fo[i * rpp:i * rpp + cm[i, 1]] for i in range(pushes)]) == 0
            want_p, want_i = path_b.numpy()[:k], idx_b.numpy()[:k]
            same = bool(k == int(cm[:, 1].sum()) and np.array_equal(got_p[ok].view(np.uint64), want_p[ok].view(np.uint64)) and np.array_equal(got_i[ok], want_i[ok]))
            for side in per:
                emit(rows, case="push", side=side, kmax=kmax, frames_per_push=fpp, pushes=pushes, **spread(per[side]))
            o, b = statistics.median(per["online"]), statistics.median(per["rerun"])
            emit(rows, case="push", side="verdict", kmax=kmax, frames_per_push=fpp, online_over_rerun=round(o / b, 4), committed_rows=k,
                 forced_rows=int((~ok).sum()), max_pending_frames=int(cm[:, 3].max()), mean_pending_frames=round(float(cm[:, 3].mean()), 2),
                 same_bits_on_committed_rows=same)
            ps.close()
            for d in (cand, cnt, st, pk, path, idx, forced, com, path_b, idx_b):
                d.free()


def large_case(pkg, vb, rows, args):
    F = args.large_frames
    for kmax in (4, 15):
        cand, cnt, st, pk = speech_lists(pkg, vb, F, kmax)
        path, idx, forced, com = vb.empty((MP + F, 2)), vb.empty(MP + F, np.int32), vb.empty(MP + F, np.uint8), vb.empty(4, np.int64)
        path_b, idx_b = vb.empty((F, 2)), vb.empty(F, np.int32)
        par = pkg.PitchPathParams.make(time_step=H / SR, silence_threshold=0.0)
        seq = pkg.PitchPathParams.make(time_step=H / SR, silence_threshold=0.0, chunk_frames=F)
        ps = vb.path_stream(kmax, par, max_pending=MP)
        res = {}
        for name in ("online", "resident_sequential", "resident_chunked"):
            ms = []
            for r in range(args.warmup + args.runs):
                vb.sync()
                vb.profile(True)
                vb.profile_reset()
                if name == "online":
                    ps.reset()
                    ps.push(cand, cnt, st, None, n_frames=F, end_utterance=True, out=(path, idx, forced, com))
                else:
                    vb.pitch_path(cand, cnt, st, None, params=seq if name == "resident_sequential" else par, n_frames=F, kmax=kmax, out=(path_b, idx_b))
                vb.sync()
                rep = vb.profile_report()
                vb.profile(False)
                if r >= args.warmup:
                    ms.append(sum(v[0] for k, v in rep.items() if k.startswith("pitch_path")))
            res[name] = ms
            emit(rows, case="large", side=name, kmax=kmax, frames=F, **spread(ms), m_frames_per_s=round(F / statistics.median(ms) / 1e3, 3),
                 ns_per_frame=round(statistics.median(ms) * 1e6 / F, 1))
        c = com.numpy()
        same = bool(c[1] == F and np.array_equal(path.numpy()[:F].view(np.uint64), path_b.numpy().view(np.uint64)) and np.array_equal(idx.numpy()[:F], idx_b.numpy()))
        emit(rows, case="large", side="verdict", kmax=kmax, frames=F, same_bits=same, forced_rows=int(c[2]))
        ps.close()
        for d in (cand, cnt, st, pk, path, idx, forced, com, path_b, idx_b):
            d.free()


def _session(pkg, vb, kmax, hops=1):
    est = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    params, ext = pkg.AnalysisParams.make(SR, formant_order=12, est_init=est), pkg.AnalysisExt.make(rms=True)
    track = pkg.PitchTrackParams.make(kmax=kmax, silence_threshold=0.0)
    rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    sess = vb.session(params, ext, track, format=pkg.SAMPLE_PCM16, frame_len=N, stride=H, max_block=max(N, hops * H))
    return sess, rec + (rec & 1)


def _pcm(vb, n):
    d = vb.synth_speech(n, sample_offset=5 * 48000 + 321)
    a = np.round(d.numpy() * (0.9 * 32767.0)).astype(np.int16)
    d.free()
    pinned = vb.malloc_host(n, np.int16)
    pinned[:] = a
    return pinned


class SessionRun:
    def __init__(self, pkg, vb, kmax, pushes):
        self.vb, self.kmax, self.pushes = vb, kmax, pushes
        self.sess, self.ld = _session(pkg, vb, kmax)
        self.audio = _pcm(vb, N + H * pushes)
        F = pushes + 1
        self.F = F
        self.out, self.st = vb.empty((F, self.ld)), vb.empty((3, F), np.int32)
        self.lists = (vb.empty((F, kmax, 2)), vb.empty(F, np.int32), vb.empty(F))
        self.path, self.idx, self.forced, self.com = vb.empty((MP + 4, 2)), vb.empty(MP + 4, np.int32), vb.empty(MP + 4, np.uint8), vb.empty(4, np.int64)

    def run(self, bound, times, sync=True):
        vb, s, k = self.vb, self.sess, self.kmax
        s.reset()
        if bound:
            s.bind_path(self.path, self.com, max_pending=MP, out_index=self.idx, out_forced=self.forced)
        pos = 0
        for i in range(self.pushes + 1):
            n = N if i == 0 else H
            lo = s.info()[1]
            outs = (self.lists[0].ptr + lo * k * 16, self.lists[1].ptr + lo * 4, self.lists[2].ptr + lo * 8, None)
            t0 = time.perf_counter()
            s.push(self.audio[pos:pos + n], out=self.out.ptr + lo * self.ld * 8, status=self.st.ptr + lo * 4, outputs=outs, record_ld=self.ld, status_ld=self.F)
            if sync:
                vb.sync()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
            pos += n

    def close(self):
        self.sess.close()
        for d in (self.out, self.st, self.path, self.idx, self.forced, self.com) + self.lists:
            d.free()
        self.vb.free_host(self.audio)


def session_case(pkg, vb, rows, args):
    for kmax in (4, 15):
        r = SessionRun(pkg, vb, kmax, args.pushes)
        per = {"bound": [], "unbound": []}
        for i in range(args.warmup + args.runs):
            for side in ("bound", "unbound"):
                t = []
                r.run(side == "bound", t)
                if i >= args.warmup:
                    per[side].append(statistics.median(t))
        for side in per:
            emit(rows, case="session", side=side, kmax=kmax, hops_per_push=1, pushes=args.pushes, **spread(per[side]))
        b, u = statistics.median(per["bound"]), statistics.median(per["unbound"])
        emit(rows, case="session", side="verdict", kmax=kmax, added_ms=round(b - u, 4), bound_over_unbound=round(b / u, 4),
             larger_spread_ms=round(max(max(v) - min(v) for v in per.values()), 4))
        r.close()


def delay_case(pkg, vb, rows, args):
    gold = os.path.join(HERE, "tests", "golden")
    for name, n, h in (("short_sample", 1024, 512), ("down_sampled", 1024, 256), ("sample-two_vowels", 1024, 512)):
        with wave.open(os.path.join(gold, name + ".wav"), "rb") as w:
            sr = float(w.getframerate())
            x = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float64) / 32767.0
        F = pkg.frame_count(x.size, n, h)
        for kmax in (4, 15):
            cand, cnt, st, pk = speech_lists(pkg, vb, F, kmax, x=x, sr=sr, n=n, h=h)
            par = pkg.PitchPathParams.make(time_step=h / sr)
            com = vb.empty((F, 4), np.int64)
            path, idx, forced = vb.empty((MP + 1, 2)), vb.empty(MP + 1, np.int32), vb.empty(MP + 1, np.uint8)
            with vb.path_stream(kmax, par, peak_ref=1.0, max_pending=MP) as ps:
                for t in range(F):
                    ps.push(cand.ptr + t * kmax * 16, cnt.ptr + 4 * t, st.ptr + 4 * t, pk.ptr + 8 * t, n_frames=1, out=(path, idx, forced, com.ptr + 32 * t))
                vb.sync()
            c = com.numpy()
            emit(rows, case="delay", recording=name, frame_len=n, stride=h, frames=F, kmax=kmax, max_pending_frames=int(c[:, 3].max()),
                 mean_pending_frames=round(float(c[:, 3].mean()), 2), forced_rows=int(c[:, 2].sum()))
            for d in (cand, cnt, st, pk, com, path, idx, forced):
                d.free()


def trace(pkg, vb, args):
    r = SessionRun(pkg, vb, 4, 2 * args.pushes)                # the first half warms, the second half is what --count-trace counts
    r.run(True, [])
    r.close()
    print(json.dumps({"case": "trace", "pushes_counted": args.pushes}), flush=True)


def count_trace(path, args, rows):
    with open(path) as f:
        disp = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in disp]
    dur = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in disp]
    ingests = [i for i, n in enumerate(names) if "session_ingest_kernel" in n]
    assert len(ingests) >= args.pushes, (len(ingests), args.pushes)
    a = ingests[-args.pushes]
    by_name, ns = {}, {}
    for n, d in zip(names[a:], dur[a:]):
        m = re.search(r"([A-Za-z_0-9]+)(<[^()]*>)?\(", n.replace("(anonymous namespace)", ""))
        short = m.group(1) if m else n
        by_name[short] = by_name.get(short, 0) + 1
        ns.setdefault(short, []).append(d)
    emit(rows, case="launches", side="bound", hops_per_push=1, pushes=args.pushes, kernel_launches_per_push=round(len(names[a:]) / args.pushes, 2),
         per_kernel={k: round(v / args.pushes, 2) for k, v in sorted(by_name.items())},
         pp_online_kernel_median_us=round(statistics.median(ns.get("pp_online_kernel", [0])) / 1e3, 2),
         smallest_other_kernel_median_us=round(min(statistics.median(v) for k, v in ns.items() if k != "pp_online_kernel") / 1e3, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--large-frames", type=int, default=360_000, help="one hour at a 10 ms hop")
    ap.add_argument("--only", choices=["push", "large", "session", "delay"], default=None)
    ap.add_argument("--trace", action="store_true")
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
            if args.trace:
                trace(pkg, vb, args)
            else:
                for name, fn in (("push", push_case), ("large", large_case), ("session", session_case), ("delay", delay_case)):
                    if args.only in (None, name):
                        fn(pkg, vb, rows, args)
    if args.out and rows:
        kept = []
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
            key = lambda r: tuple(r.get(k) for k in ("case", "side", "kmax", "frames_per_push", "recording"))
            new = {key(r) for r in rows}
            kept = [r for r in old if key(r) not in new]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(kept + rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
