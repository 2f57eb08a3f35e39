#!/usr/bin/env python3
"""Which unit cells does a Brent run of the pitch refinement visit?  A CPU replay of brent_maximize (src/periodic.rs:103-188)
around the oracle's interpolate_sinc, checked bit for bit against the oracle's improve_extremum_sinc on every run it replays.

A unit cell is the interval between two integer lags: the samples one evaluation multiplies depend on the cell of its abscissa
alone, which is what improve_extremum_sinc_wave's register sets are built on (two cells kept, a third refills the older one).

usage: python3 tools/experiments/brent_cells.py [synth|glide] [--every K] [--shape N:HOP] [--all-candidates]
  synth   the synthetic recording at 1200/480 (default every 7th frame of the first 847): the top candidate with y[k] >= 0.3
  glide   the input of tests/test_gpu_refine_cell_cache.py (default every 3rd frame)
Prints per input: runs replayed / matched, evaluations per run, distinct cells per run, cell switches per run, lags, whole blocks
of four per lane, and the runs that visit a THIRD cell or take an exact-integer early-out (|x - round(x)| < 1e-10)."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as g

SR, FMIN, FMAX = 48000.0, 75.0, 600.0
GOLDEN = 1. - 0.6180339887498948482045868343656381177203091798057628621
SQRT_EPS, EPS, TOL = 1.4901161193847656e-08, 2.220446049250313e-16, 1e-10


def _hist(v):
    return {int(k): int(c) for k, c in zip(*np.unique(v, return_counts=True))}


def brent_replay(f, a, b):
    """-> (x, fx, abscissae); a MINIMISER of f, as the reference's brent_maximize is (quirk Q8)"""
    xs = []
    v = a + GOLDEN * (b - a)
    fv = f(v); xs.append(v)
    x = w = v
    fx = fw = fv
    for _ in range(60):
        rng = b - a
        mid = (a + b) * 0.5
        tol_act = SQRT_EPS * abs(x) + TOL / 3.
        if abs(x - mid) + rng * 0.5 <= 2. * tol_act:
            break
        new_step = GOLDEN * (b - x) if x < mid else GOLDEN * (a - x)
        if abs(x - w) >= tol_act:
            t = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * t
            q = 2. * q - t
            if q > 0.:
                p = -p
            else:
                q = -q
            if abs(p) < abs(new_step * q) and p > q * (a - x + 2. * tol_act) and p < q * (b - x - 2. * tol_act):
                new_step = p / q
        if abs(new_step) < tol_act:
            new_step = tol_act if new_step > 0. else -tol_act
        t = x + new_step
        ft = f(t); xs.append(t)
        if ft <= fx:
            if t < x:
                b = x
            else:
                a = x
            v, w, x = w, x, t
            fv, fw, fx = fw, fx, ft
        else:
            if t < x:
                a = t
            else:
                b = t
            if ft <= fw or abs(w - x) < EPS:
                v, w = w, t
                fv, fw = fw, ft
            elif ft <= fv or abs(v - x) < EPS or abs(v - w) < EPS:
                v = t
                fv = ft
    return x, fx, xs


def runs_of_frame(o, frame, n, all_candidates):
    """the (lag, y, offset, nx, ixmid) of the frame's runs: its candidates in 75..600 Hz, or the top one with y[k] >= 0.3"""
    w = o.window("hanning", n)
    wl = o.window("hanning_lag", n)
    r = o.normalize(o.autocorrelate(frame * w, n))
    y = np.concatenate([r / wl, np.zeros(n)])
    b = n // 2
    offset = -b - 1
    nx = b - offset
    out = []
    for k in range(1, b - 1):
        if not (y[k - 1] < y[k] and y[k + 1] < y[k]):
            continue
        dr = 0.5 * (y[k + 1] - y[k - 1])
        d2r = 2. * y[k] - (y[k - 1] - y[k + 1])
        freq = SR / (k + dr / d2r)
        if not (FMIN < freq < FMAX):
            continue
        out.append((k, y, offset, nx, SR / freq - offset))
    if not all_candidates:
        out = sorted([c for c in out if c[1][c[0]] >= 0.3], key=lambda c: -c[1][c[0]])[:1]
    return out


def main():
    args = sys.argv[1:]
    kind = args[0] if args and not args[0].startswith("--") else "synth"
    every = int(args[args.index("--every") + 1]) if "--every" in args else (7 if kind == "synth" else 3)
    n, hop = (int(v) for v in args[args.index("--shape") + 1].split(":")) if "--shape" in args else (1200, 480)
    all_candidates = "--all-candidates" in args
    pkg = g.load_package()
    o = g.load_oracle()
    if kind == "glide":
        import test_gpu_refine_cell_cache as t
        pcm, frames = t.glide_pcm(n, hop)
        audio = pcm.astype(np.float64) / 32767.0
    else:
        synth = importlib.import_module(pkg.__name__ + ".synth")
        frames = 847
        audio = synth.synth_speech((frames - 1) * hop + n, 0)
    runs = matched = 0
    evals, cells, switches, lags, blocks, third, early = [], [], [], [], [], [], []
    for f in range(0, frames, every):
        for k, y, offset, nx, ixmid in runs_of_frame(o, audio[f * hop:f * hop + n], n, all_candidates):
            if ixmid == 0. or ixmid >= nx:
                continue
            fn = lambda x: o.interpolate_sinc(y, offset, nx, x, 1200)[1]
            x, fx, xs = brent_replay(fn, ixmid - 1., ixmid + 1.)
            st, xm, ym = o.improve_extremum_sinc(y, offset, nx, ixmid, 1200)
            runs += 1
            matched += int(st == 0 and xm == x and ym == fx)
            seq = [int(np.floor(v)) for v in xs]
            order = []
            for c in seq:
                if c not in order:
                    order.append(c)
            evals.append(len(xs)); cells.append(len(order)); lags.append(k)
            switches.append(sum(1 for i in range(1, len(seq)) if seq[i] != seq[i - 1]))
            blocks.append(((k + 1 - 31) // 32 + 1) // 4 if k + 1 >= 31 else 0)
            if len(order) > 2:
                third.append((f, k, order))
            if any(abs(v - round(v)) < 1e-10 for v in xs):
                early.append((f, k))
    if not runs:
        print(kind, "no runs"); return
    ev = np.array(evals); sw = np.array(switches)
    print("%s %d/%d every %d: runs %d, bit for bit the oracle's improve_extremum_sinc in %d" % (kind, n, hop, every, runs, matched))
    print("  evaluations per run %.1f (%d..%d); cells per run: %s; switches per run %.1f (%d..%d) = %.0f %% of evaluations"
          % (ev.mean(), ev.min(), ev.max(), _hist(cells), sw.mean(), sw.min(), sw.max(),
             100. * sw.sum() / ev.sum()))
    print("  lags %d..%d, median %d; whole blocks per lane: %s" % (min(lags), max(lags), int(np.median(lags)),
                                                                 _hist(blocks)))
    print("  runs with a third cell: %d %s" % (len(third), third[:6]))
    print("  runs with an exact-integer early-out: %d %s" % (len(early), early[:6]))


if __name__ == "__main__":
    main()
