#!/usr/bin/env python3
"""Times a bound session pool's tick (vbx_pool_path_bind) on one MI355X.  All round trips are a host clock
around a tick that ENDS IN vbx_sync; the three sides alternate in one process after a warm-up pass, and the spread of the passes is
reported with each median.  Streams: 16-bit PCM at 400 / 160, resident on the device (vbx_pool_push_device: only the tick's tables
are uploaded), every stream pushing ONE hop per tick -- the steady state of a gateway.

  a  bound      the bound pool's tick: the unbound tick's launches plus ONE pitch_path_online_pool
  b  streams    the same pool unbound plus one vbx_path_stream_push per stream on the tick's delivered lists: what a caller had before
                (the pushes are raw library calls with precomputed addresses, the cheapest form a Python caller has)
  c  unbound    the unbound tick alone

  python tools/pool_path_bench.py --out profiles/pool_path/report.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SR, N, H, MP = 48000.0, 400, 160, 64


def emit(rows, **r):
    print(json.dumps(r), flush=True)
    rows.append(r)


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "runs": len(v)}


class Side:
    """one pool of n streams and its tick outputs; bound: to its own contour arrays; streams: one PathStream per slot"""

    def __init__(self, pkg, vb, n, kmax, audio, offs, ticks, kind):
        self.pkg, self.vb, self.n, self.kmax, self.audio, self.offs, self.kind = pkg, vb, n, kmax, audio, offs, kind
        est = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
        params = pkg.AnalysisParams.make(SR, est_init=est)
        self.track = pkg.PitchTrackParams.make(kmax=kmax)
        rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), None))
        self.ld = rec + (rec & 1)
        self.pool = vb.pool(params, None, self.track, format=pkg.SAMPLE_PCM16, frame_len=N, stride=H, max_streams=n, max_block=N, max_tick=n * N)
        cap = n * (N // H + 1)
        self.cap = cap
        self.rec, self.st = vb.empty((cap, self.ld)), vb.empty((3, cap), np.int32)
        self.lists = (vb.empty((cap, kmax, 2)), vb.empty(cap, np.int32), vb.empty(cap))
        self.kw = dict(out=self.rec.ptr, status=self.st.ptr, outputs=tuple(d.ptr for d in self.lists) + (None,), record_ld=self.ld, status_ld=cap)
        self.own = [self.rec, self.st] + list(self.lists)
        self.pos = 0
        if kind == "bound":
            R = pkg.pool_path_slot_rows(MP, N, H)
            self.path, self.idx, self.forced, self.com = vb.empty((n * R, 2)), vb.empty(n * R, np.int32), vb.empty(n * R, np.uint8), vb.empty((n, 4), np.int64)
            self.pool.bind_path(self.path, self.com, max_pending=MP, slot_rows=R, out_index=self.idx, out_forced=self.forced)
            self.own += [self.path, self.idx, self.forced, self.com]
        if kind == "streams":
            R = MP + N // H + 1
            par = type(self.track.path).from_buffer_copy(self.track.path)
            par.time_step = H / SR                             # (the tracked call's meaning of time_step == 0)
            self.ps = [vb.path_stream(kmax, par, peak_ref=1.0, max_pending=MP) for _ in range(n)]
            self.path, self.idx, self.forced, self.com = vb.empty((n * R, 2)), vb.empty(n * R, np.int32), vb.empty(n * R, np.uint8), vb.empty((n, 4), np.int64)
            self.own += [self.path, self.idx, self.forced, self.com]
            self.dst = [(self.path.ptr + 16 * k * R, self.idx.ptr + 4 * k * R, self.forced.ptr + k * R, self.com.ptr + 32 * k) for k in range(n)]
        self.tick(N)                                           # the first block of every stream: one frame each

    def tick(self, size=H):
        vb, a = self.vb, self.audio.ptr
        ents = [(k, a + 2 * (self.offs[k] + self.pos), size) for k in range(self.n)]
        t0 = time.perf_counter()
        rows, total = self.pool.push_device(ents, **self.kw)
        if self.kind == "streams":
            push, c, cn, st, pk, km = vb.L.vbx_path_stream_push, self.lists[0].ptr, self.lists[1].ptr, self.st.ptr, self.lists[2].ptr, self.kmax
            for k in range(self.n):
                r0, nr = int(rows[k, 0]), int(rows[k, 1])
                d = self.dst[k]
                vb._check(push(self.ps[k].handle, c + 16 * km * r0, cn + 4 * r0, st + 4 * r0, pk + 8 * r0, nr, 0, d[0], 2, d[1], d[2], d[3]))
        vb.sync()
        self.pos += size
        return (time.perf_counter() - t0) * 1e3

    def contour_rows(self):
        """(commit records [n, 4], the rows of the last tick) -- the two forms must agree"""
        return self.com.numpy(), self.path.numpy()

    def close(self):
        if self.kind == "streams":
            for p in self.ps:
                p.close()
        self.pool.close()
        for d in self.own:
            d.free()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=30, help="ticks per pass")
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    rows = []
    with pkg.VoxBox(0) as vb:
        total_ticks = (args.warmup + args.runs) * args.ticks
        span = N + H * total_ticks
        for n in args.streams:
            offs = [(k * 37) % 4001 for k in range(n)]
            d = vb.synth_speech(span + 4001, sample_offset=5 * 48000 + 321)
            audio = vb.to_device(np.round(d.numpy() * (0.9 * 32767.0)).astype(np.int16), np.int16)
            d.free()
            for kmax in (4, 15):
                sides = {k: Side(pkg, vb, n, kmax, audio, offs, total_ticks, k) for k in ("bound", "streams", "unbound")}
                per = {k: [] for k in sides}
                for r in range(args.warmup + args.runs):
                    for k, s in sides.items():                 # the sides alternate pass by pass
                        t = [s.tick() for _ in range(args.ticks)]
                        if r >= args.warmup:
                            per[k].append(statistics.median(t))
                ca, pa = sides["bound"].contour_rows()
                cb, pb = sides["streams"].contour_rows()
                Ra, Rb = pa.shape[0] // n, pb.shape[0] // n
                same = bool(np.array_equal(ca, cb) and all(np.array_equal(pa[k * Ra:k * Ra + ca[k, 1]].view(np.uint64), pb[k * Rb:k * Rb + cb[k, 1]].view(np.uint64))
                                                           for k in range(n)))
                for k in per:
                    emit(rows, case="tick", side=k, streams=n, kmax=kmax, hops_per_tick=1, ticks_per_pass=args.ticks, **spread(per[k]))
                a, b, c = (statistics.median(per[k]) for k in ("bound", "streams", "unbound"))
                emit(rows, case="tick", side="verdict", streams=n, kmax=kmax, bound_minus_unbound_ms=round(a - c, 4), streams_minus_unbound_ms=round(b - c, 4),
                     bound_over_unbound=round(a / c, 4), streams_over_unbound=round(b / c, 4), same_commits_and_rows_in_the_last_tick=same)
                for s in sides.values():
                    s.close()
            audio.free()
    if args.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
