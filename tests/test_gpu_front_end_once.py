"""The candidate front end of the fused kernel with each value computed once (pitch_refine_store<.., ONCE>: block sums of |y|
kept between the two prefix loops, the quad bound pass's abscissa read back by the refinement, pick_best_pred's ballot),
pinned bit for bit to the build BEFORE it, at 1200/480 and 1024/512, on 596 frames that walk the number of candidates through
every path of the front end: sha-256 of
  * the FUSED kernel's own lists, counts, peaks, path indices, records and statuses at kmax 1, 2, 3 and 4
    (vbx_analyze_frames_tracked_f64 with lists: at 1200/480 this is the instance that takes the new form, and the only way to
    run it with a list longer than one; kmax 4 takes the group path),
  * the plain fused record (kmax = 1 by construction), and
  * vbx_pitch_f64's lists, counts and statuses at kmax 1, 2 and 3.  (At 1200/480 vbx_pitch_f64 runs an instance that keeps the
    plain form, and 1024/512 takes a power-of-two plan, plain too: these digests hold what this change must NOT touch.)

Input (front_end_pcm), per shape (periods below are those at 1200 samples; they scale with the frame length):
  * three glides of a tone's PERIOD (the lag curve of a tone of period P peaks at every multiple of P, and the filter keeps
    lags from 80 = 48 kHz / 600 Hz on): 3.4 .. 10 samples (more than 128 candidates down to ~50: the peak count crosses 128
    and 64, the candidate count 65, 64, 63, i.e. one 64-lane pass or two, and the quad / lane-per-candidate switch),
    26 .. 42 samples (19 .. 11 candidates: the quad pass's first round of 16 holds all of them, or not), and 150 .. 1500
    samples (3, 2, 1 and 0 candidates);
  * a tone with two harmonics under noise (a winner that is not the first candidate);
  * silence, then silence written as -0.0, then one impulse in silence.
  Weak noise (an integer hash) lies under the glides so that no stretch of a curve is flat.  The samples are quantised to
  16 bits before anything is computed from them; the -0.0 stretch is applied to the f64 samples afterwards.

What must occur is ASSERTED on the outputs (test_the_input_reaches_every_class), not assumed: candidate counts (the frame's
count less the unvoiced entry) of exactly 0, 1, 15, 16, 17, 63, 64, 65 and above 128 at each shape -- a count above 128 /
above 64 is that many PEAKS at least, so the peak count crosses both; on the FUSED kernel's lists at kmax = 3: a frame whose
top entry is not its first candidate (a later entry has a higher frequency, i.e. a lower lag, than the top's) and a frame
whose three entries hold two refined candidates while more remain (both had to be refined to the end); the fused kernel's
counts equal vbx_pitch_f64's; an all-zero frame, an all -0.0 frame and an impulse frame, found by their samples.

tests/golden/front_end_once_digests.json holds the digests of the PARENT build; tools/record_front_end_once_digests.py
writes it (only ever from a build whose outputs are the accepted ones).

Needs a real MI355X: run with `-m gpu`.
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 48000.0
SHAPES = [(1200, 480), (1024, 512)]
KMAX = (1, 2, 3)
KMAX_FUSED = (1, 2, 3, 4)                                    # lists of the fused kernel itself (the tracked call); 4: the group path
FRAMES = 596
GOLDEN = "front_end_once_digests.json"
CLASSES = (0, 1, 15, 16, 17, 63, 64, 65)
# (frames, period from, period to): geometric glides of the tone's period, in samples
GLIDES = ((330, 3.4, 10.0), (130, 26.0, 42.0), (90, 150.0, 1500.0))
TAIL = (("harmonics", 16), ("silence", 10), ("minus_zero", 10), ("impulse", 10))     # name, frames


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hash_noise(count, seed):
    """uniform in [-1, 1), a pure integer hash of the sample index (splitmix64): the same on every host"""
    with np.errstate(over="ignore"):
        z = np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


def front_end_pcm(n, hop):
    """-> (f64 samples, int16 samples, {name: (first frame, frames)}) of FRAMES frames of n samples, hop apart"""
    assert sum(g[0] for g in GLIDES) + sum(t[1] for t in TAIL) == FRAMES
    total = (FRAMES - 1) * hop + n
    x = np.zeros(total)
    where = {}
    f0 = 0
    for gi, (frames, p_from, p_to) in enumerate(GLIDES):
        a, b = f0 * hop, min((f0 + frames) * hop, total)
        t = np.arange(b - a, dtype=np.float64) / float(b - a)
        period = (n / 1200.0) * p_from * (p_to / p_from) ** t      # the searched lags scale with the frame
        phase = 2.0 * np.pi * np.cumsum(1.0 / period)
        x[a:b] = 0.6 * np.sin(phase) + 0.002 * _hash_noise(b - a, 0xF00D + gi)
        where["glide%d" % gi] = (f0, frames)
        f0 += frames
    for name, frames in TAIL:
        a, b = f0 * hop, min((f0 + frames) * hop + n, total)
        if name == "harmonics":
            b = (f0 + frames) * hop
            s = np.arange(b - a, dtype=np.float64)
            ph = 2.0 * np.pi * s / 97.3
            x[a:b] = 0.3 * np.sin(ph) + 0.25 * np.sin(2.0 * ph + 0.4) + 0.2 * np.sin(3.0 * ph + 1.1) + 0.05 * _hash_noise(b - a, 0xBEEF)
        elif name == "impulse":
            x[a:b] = 0.0
            x[a + 4 * hop + n // 2] = 0.8                     # inside frame f0 + 4, whatever the shape
        else:
            x[a:b] = 0.0
        where[name] = (f0, frames)
        f0 += frames
    pcm = np.round(x * 32767.0 * 0.9).astype(np.int16)
    xq = pcm.astype(np.float64) / 32767.0
    z0, zf = where["minus_zero"]
    a, b = z0 * hop, (z0 + zf) * hop
    assert not xq[a:b].any()
    xq[a:b] = -0.0
    return xq, pcm, where


def _params(pkg):
    return pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=0, mfcc=(13, 100.0, 8000.0))


def run_shape(vb, pkg, n, hop):
    """every output the digests cover, plus the whole lists (kmax = 64) the class assertions read"""
    x, _, where = front_end_pcm(n, hop)
    audio = vb.to_device(x)
    han = vb.window(pkg.WINDOW_HANNING, n)
    out = {"x": x, "where": where}
    for k in KMAX + (64,):
        out["k%d" % k] = vb.pitch(audio, SR, 0.2, 75.0, 600.0, kmax=k, frame_len=n, stride=hop, n_frames=FRAMES, window=han)
    params = _params(pkg)
    out["record"] = vb.analyze_frames(audio, params, frame_len=n, stride=hop, n_frames=FRAMES)
    for k in KMAX_FUSED:                                     # (records, status3, cand [F, k, 2], count, peak, index)
        out["fused_k%d" % k] = vb.analyze_frames_tracked(audio, params, pkg.PitchTrackParams.make(kmax=k), frame_len=n, stride=hop,
                                                         n_frames=FRAMES, lists=True)
    out["columns"] = params.columns()
    audio.free()
    return out


def digests_of(out):
    d = {"frames": FRAMES}
    for k in KMAX:
        cand, cnt, st = out["k%d" % k]
        assert cand.shape == (FRAMES, k, 2)
        d["pitch_k%d" % k] = _sha(cand)
        d["count_k%d" % k] = _sha(cnt)
        d["status_k%d" % k] = _sha(st)
    rec, st3 = out["record"]
    for name, (c0, w) in out["columns"].items():
        d["record_" + name] = _sha(rec[:, c0:c0 + w])
    d["record_status"] = _sha(st3)
    for k in KMAX_FUSED:
        rec, st3, cand, cnt, peak, index = out["fused_k%d" % k]
        assert cand.shape == (FRAMES, k, 2)
        for name, a in (("record", rec), ("status", st3), ("lists", cand), ("count", cnt), ("peak", peak), ("index", index)):
            d["fused_k%d_%s" % (k, name)] = _sha(a)
    return d


def compute_digests(vb, pkg):
    return {"front end %d/%d" % (n, hop): digests_of(_run_cached(vb, pkg, n, hop)) for n, hop in SHAPES}


_RUNS = {}


def _run_cached(vb, pkg, n, hop):
    if (n, hop) not in _RUNS:
        _RUNS[(n, hop)] = run_shape(vb, pkg, n, hop)
    return _RUNS[(n, hop)]


@pytest.mark.parametrize("n,hop", SHAPES)
def test_the_input_reaches_every_class(vb, pkg, n, hop):
    out = _run_cached(vb, pkg, n, hop)
    x, where = out["x"], out["where"]
    cand1, cnt1, st1 = out["k1"]
    cand3, cnt3, _ = out["k3"]
    cand64, cnt64, _ = out["k64"]
    assert not st1.any()
    ncand = cnt1.astype(np.int64) - 1                        # less the unvoiced entry of :452
    print("%d/%d candidates per frame: min %d max %d; frames per class:" % (n, hop, ncand.min(), ncand.max()),
          {c: int(np.sum(ncand == c)) for c in CLASSES}, "above 128:", int(np.sum(ncand > 128)))
    for c in CLASSES:
        assert np.any(ncand == c), "no frame with %d candidates" % c
    assert np.any(ncand > 128)                               # at least that many peaks: the peak count crosses 64 and 128 ...
    assert np.any((ncand > 64) & (ncand <= 128)) and np.any(ncand < 64)   # ... from both sides
    assert np.array_equal(cnt1, cnt3) and np.array_equal(cnt1, cnt64)
    # the same classes in the fused kernel itself, and these two on ITS lists at kmax = 3
    fused3, fcnt3 = out["fused_k3"][2], out["fused_k3"][3]
    for k in KMAX_FUSED:
        assert np.array_equal(out["fused_k%d" % k][3], cnt1), "fused kernel's counts at kmax %d" % k
    # a winner that is not the first candidate (candidate 0 has the lowest lag = the highest frequency): a later entry is higher
    top_f = fused3[:, 0, 0]
    not_first = (ncand >= 2) & (top_f > 0.0) & (fused3[:, 1:, 0].max(axis=1) > top_f)
    print("fused kernel, frames whose winner is not candidate 0:", int(not_first.sum()))
    assert not_first.any()
    # two candidates refined to the end: both returned at kmax = 3 (beside the unvoiced entry or above it), more were there
    two = (ncand >= 3) & (np.sum(fused3[:, :, 0] > 0.0, axis=1) >= 2)
    print("fused kernel, frames with two refined candidates returned:", int(two.sum()))
    assert two.any()
    # ... in frames the quad pass's kept abscissas serve (at most 16 candidates) and in frames beyond them
    assert np.any(two & (ncand <= 16)) and np.any(two & (ncand > 16) & (ncand <= 32))
    # the three degenerate frames, by their samples
    fr = np.lib.stride_tricks.sliding_window_view(x, n)[::hop][:FRAMES]
    silent = [f for f in range(*_span(where["silence"])) if not fr[f].any() and not np.signbit(fr[f]).any()]
    minus = [f for f in range(*_span(where["minus_zero"])) if not fr[f].any() and np.signbit(fr[f]).all()]
    impulse = [f for f in range(*_span(where["impulse"])) if np.count_nonzero(fr[f]) == 1]
    print("silent", silent, "-0.0", minus, "impulse", impulse)
    assert silent and minus and impulse


def _span(w):
    return w[0], w[0] + w[1]


def test_front_end_outputs_keep_the_parent_builds_digests(vb, pkg, golden_dir):
    with open(os.path.join(golden_dir, GOLDEN)) as f:
        want = json.load(f)["digests"]
    got = compute_digests(vb, pkg)
    assert sorted(got) == sorted(want)
    differ = ["%s: %s" % (shape, k) for shape in want for k in want[shape] if got[shape].get(k) != want[shape][k]]
    for shape in want:
        print(shape, want[shape]["frames"], "frames:", "identical" if not any(s.startswith(shape + ":") for s in differ) else "DIFFER")
    assert not differ, differ
    assert all(sorted(got[s]) == sorted(want[s]) for s in want)
