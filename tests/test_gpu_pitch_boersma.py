"""vbx_pitch_boersma_f64 on the device against the numpy model of its definition (tests/pitch_boersma_model.py), against a
long-double evaluation of the interpolant at the lags it returns (independent of the model's Brent run), and into the pitch path.

Device samples are pulled back, so both sides see the same input.  On frames the model does not flag (no decision within 1e-9 of
flipping) out_count, status, which entries are selected and their order must be exact, Hz within 1e-4 |b| and strengths within
1e-6 (BASELINE's parity metric).  Flagged frames are counted, reported, and compared on count and status only.  The worst
observed differences go to the report (a file when VBX_TEST_REPORT_DIR is set; profiles/pitch_boersma/report.json is one)."""
import ctypes as C
import json
import os
import wave

import numpy as np
import pytest

import layout_arena as la
import pitch_boersma_model as M
import pitch_path_model as PM

pytestmark = pytest.mark.gpu

SR = 48000.0
TH, FMIN, FMAX = 0.2, 75.0, 600.0
NOISE_AT = 4 * 48000 - 2400              # frames that run into second 4 of the synthetic signal: noise, > 63 candidates a frame
REPORT = {"cases": {}, "worst_hz_rel": 0.0, "worst_strength_abs": 0.0, "flagged_frames": 0, "frames": 0,
          "worst_deficit": -1.0, "worst_strength_vs_longdouble": 0.0}


def _read_wav16(path):
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 1
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        return pcm.astype(np.float64) / 32767.0, float(w.getframerate())


@pytest.fixture(scope="module")
def signals(vb, golden_dir):
    """name -> (samples, sample rate): the device's synthetic signal pulled back (voiced from offset 0, noise across second 4), a
    recording."""
    d = vb.synth_speech(40000, sample_offset=0)
    voiced = d.numpy()
    d.free()
    d = vb.synth_speech(40000, sample_offset=NOISE_AT)
    noise = d.numpy()
    d.free()
    wav, wsr = _read_wav16(os.path.join(golden_dir, "sample-two_vowels.wav"))
    return {"voiced": (voiced, SR), "noise": (noise, SR), "vowels": (wav, wsr)}


def _window(vb, pkg, n, use):
    return (vb.window(pkg.WINDOW_HANNING, n), pkg.window_table(pkg.WINDOW_HANNING, n)) if use else (None, None)


_MODEL = {}


def _model(key, x, F, N, S, w, sr, fmin, fmax, kmax):
    """The model's answer, computed once per (input, shape, kmax) and left unchanged."""
    if key not in _MODEL:
        _MODEL[key] = M.pitch_boersma(x, F, N, S, w, sr, TH, fmin, fmax, kmax)
    return _MODEL[key]


def _compare(name, got, want, sr):
    """got / want: (cand, count, status[, results]).  Returns the number of flagged frames."""
    cand, count, status = got
    mc, mn, ms, res = want
    assert np.array_equal(count, mn), (name, np.nonzero(count != mn)[0][:8], count[:8], mn[:8])
    assert np.array_equal(status, ms), (name, np.nonzero(status != ms)[0][:8])
    flagged, whz, wst = 0, 0.0, 0.0
    for t, r in enumerate(res):
        if r.flagged:
            flagged += 1
            continue
        a, b = cand[t], mc[t]
        # which entries and in which order: a voiced slot is voiced in both and lands on the same peak (within half a lag of the model's)
        assert np.array_equal(a[:, 0] == 0.0, b[:, 0] == 0.0), (name, t, a, b)
        v = b[:, 0] > 0.0
        dhz = np.abs(a[v, 0] - b[v, 0]) / np.abs(b[v, 0]) if v.any() else np.zeros(0)
        dst = np.abs(a[:, 1] - b[:, 1])
        print(f"{name} frame {t}: worst Hz rel {dhz.max() if dhz.size else 0.0:.3e}, worst strength abs {dst.max():.3e}")
        assert np.all(dhz <= 1e-4), (name, t, a, b)
        assert np.all(dst <= 1e-6), (name, t, a, b)
        whz, wst = max(whz, float(dhz.max()) if dhz.size else 0.0), max(wst, float(dst.max()))
    REPORT["cases"][name] = dict(frames=len(res), flagged=flagged, worst_hz_rel=whz, worst_strength_abs=wst,
                                 mean_count=float(np.mean(mn)), max_count=int(np.max(mn)))
    REPORT["worst_hz_rel"] = max(REPORT["worst_hz_rel"], whz)
    REPORT["worst_strength_abs"] = max(REPORT["worst_strength_abs"], wst)
    REPORT["flagged_frames"] += flagged
    REPORT["frames"] += len(res)
    assert flagged <= 0.01 * len(res) or flagged <= 0, (name, "flagged share above 1 %", flagged, len(res))
    return flagged


# (name, signal, frame_len, stride, n_frames, kmax, window, fmax): the smallest shapes that cross each seam -- single-pass lengths
# with y in the image's place (16 .. 1280), two-region lengths (1281, 2048, 4096), frame counts that are no multiple of the XCD
# count, every kmax class, the noise stretch whose frames carry more than 63 candidates (selection and the LDS list), a
# recording, the hop-strided view and dense batches, with and without a window.  Short frames take a ceiling their lags can reach.
CASES = [
    ("voiced-1200-k15", "voiced", 1200, 480, 63, 15, True, FMAX),
    ("voiced-1200-k1-F1", "voiced", 1200, 480, 1, 1, True, FMAX),
    ("voiced-1200-k2-nowin", "voiced", 1200, 480, 9, 2, False, FMAX),
    ("noise-1200-k4", "noise", 1200, 480, 31, 4, True, FMAX),
    ("noise-1200-k1", "noise", 1200, 480, 9, 1, True, FMAX),
    ("noise-1200-k63", "noise", 1200, 480, 9, 63, True, FMAX),
    ("voiced-16-k4", "voiced", 16, 16, 63, 4, True, 30000.0),
    ("voiced-64-k2-F257", "voiced", 64, 64, 257, 2, False, 30000.0),
    ("voiced-1103-k15", "voiced", 1103, 480, 5, 15, True, FMAX),
    ("voiced-1280-k4", "voiced", 1280, 1280, 5, 4, True, FMAX),
    ("voiced-1281-k4", "voiced", 1281, 480, 5, 4, True, FMAX),
    ("noise-2048-k15", "noise", 2048, 2048, 5, 15, False, FMAX),
    ("voiced-4096-k15", "voiced", 4096, 480, 3, 15, True, FMAX),
    ("vowels-1024-k15", "vowels", 1024, 512, 33, 15, True, FMAX),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matches_the_model(vb, pkg, signals, case):
    name, sig, N, S, F, kmax, use_win, fmax = case
    x, sr = signals[sig]
    x = x[:(F - 1) * S + N]
    assert x.size == (F - 1) * S + N
    dw, hw = _window(vb, pkg, N, use_win)
    if S == N:                                                  # a dense [F, N] batch
        got = vb.pitch_boersma(x.reshape(F, N), sr, TH, FMIN, fmax, kmax=kmax, window=dw)
    else:                                                       # the hop-strided view
        got = vb.pitch_boersma(x, sr, TH, FMIN, fmax, kmax=kmax, frame_len=N, stride=S, n_frames=F, window=dw)
    want = _model(case, x, F, N, S, hw, sr, FMIN, fmax, kmax)
    _compare(name, got, want, sr)
    if sig == "noise" and N == 1200:
        assert int(np.max(want[1])) > 63, "the noise stretch no longer exercises selection"


def test_returned_lags_are_local_maxima_of_the_long_double_interpolant(vb, pkg, signals):
    """Independent of the model's Brent run: at every voiced entry the device returns, S_ld(sample_rate / frequency) is within 1e-9
    of the largest of S_ld at the nearest integer lag and at +-1e-3 lags (Brent stops within 2 tol_act ~ 1e-5 lags of a stationary
    point of a band-limited curve with |S''| of a few units: a deficit of order 1e-10), and its reflected value is the returned
    strength to 1e-6."""
    hw = pkg.window_table(pkg.WINDOW_HANNING, 1200)
    dw = vb.window(pkg.WINDOW_HANNING, 1200)
    for sig, F, kmax in (("voiced", 12, 15), ("noise", 4, 8)):
        x, sr = signals[sig]
        x = x[:(F - 1) * 480 + 1200]
        cand, count, status = vb.pitch_boersma(x, sr, TH, FMIN, FMAX, kmax=kmax, frame_len=1200, stride=480, n_frames=F, window=dw)
        assert np.all(status == 0)
        for t in range(F):
            y = M.curve(x[t * 480:t * 480 + 1200] * hw)
            for fq, st in cand[t]:
                if fq <= 0.0:
                    continue
                deficit, here = M.local_max_deficit(y, sr / fq)
                print(f"{sig} frame {t} {fq:.4f} Hz: deficit {deficit:.3e}, strength - S_ld {st - M.reflect(here):.3e}")
                REPORT["worst_deficit"] = max(REPORT["worst_deficit"], deficit)
                REPORT["worst_strength_vs_longdouble"] = max(REPORT["worst_strength_vs_longdouble"], abs(st - M.reflect(here)))
                assert deficit <= 1e-9, (sig, t, fq, deficit)
                assert abs(st - M.reflect(here)) <= 1e-6, (sig, t, fq, st, here)


# at least three periods in the frame; the integer lag next to the peak is off by 1.1e-3 .. 1.7e-3
TONES = [(1200, 48000.0, 211.7, 1), (1200, 48000.0, 433.1, 1), (1200, 48000.0, 137.3, 7), (1200, 48000.0, 211.7, 7),
         (1024, 44100.0, 211.7, 1), (1024, 44100.0, 433.1, 1), (1024, 44100.0, 311.3, 7), (1024, 44100.0, 211.7, 7)]


def tone(n, sr, f0, harmonics):
    t = np.arange(n) / sr
    return sum(np.sin(2.0 * np.pi * f0 * h * t) / h for h in range(1, harmonics + 1))


def test_tones_through_the_c_abi(vb, pkg):
    """The sine and harmonic frames: the top voiced candidate within 1e-4 relative of f0 (BASELINE's Hz tolerance), and at least ten
    times closer than the integer lag vbx_pitch_f64 returns for the same frame."""
    for n, sr, f0, harm in TONES:
        x = tone(n, sr, f0, harm)[None, :]
        dw = vb.window(pkg.WINDOW_HANNING, n)
        cand, count, status = vb.pitch_boersma(x, sr, TH, FMIN, FMAX, kmax=4, window=dw)
        ref, _, _ = vb.pitch(x, sr, TH, FMIN, FMAX, kmax=4, window=dw)
        assert status[0] == 0 and cand[0, 0, 0] > 0.0
        err, err_ref = abs(cand[0, 0, 0] - f0) / f0, abs(ref[0, 0, 0] - f0) / f0
        print(f"{n} @ {sr}: f0 {f0} x{harm}: {cand[0, 0, 0]:.5f} Hz (rel {err:.2e}); vbx_pitch_f64 {ref[0, 0, 0]:.5f} (rel {err_ref:.2e})")
        assert err <= 1e-4, (n, sr, f0, harm, cand[0, 0])
        assert err * 10.0 <= err_ref, (n, sr, f0, harm, cand[0, 0], ref[0, 0])


def test_two_runs_are_bit_identical(vb, pkg, signals):
    x, sr = signals["noise"]
    F = 40
    dw = vb.window(pkg.WINDOW_HANNING, 1200)
    for kmax in (1, 4, 15):
        a = vb.pitch_boersma(x, sr, TH, FMIN, FMAX, kmax=kmax, frame_len=1200, stride=480, n_frames=F, window=dw)
        b = vb.pitch_boersma(x, sr, TH, FMIN, FMAX, kmax=kmax, frame_len=1200, stride=480, n_frames=F, window=dw)
        for u, v, nm in zip(a, b, ("cand", "count", "status")):
            la.assert_same_bits(f"kmax {kmax}", nm, u, v)


def test_whole_list_does_not_change_with_kmax(vb, pkg, signals):
    """kmax >= out_count: the row is the frame's whole list, whatever kmax (bit for bit among kmax >= 4, the class these share)."""
    x, sr = signals["voiced"]
    F = 40
    dw = vb.window(pkg.WINDOW_HANNING, 1200)
    big = vb.pitch_boersma(x, sr, TH, FMIN, FMAX, kmax=63, frame_len=1200, stride=480, n_frames=F, window=dw)
    top = int(big[1].max())
    assert 4 <= top <= 40
    for kmax in (top, top + 1, 41):
        c, n, s = vb.pitch_boersma(x, sr, TH, FMIN, FMAX, kmax=kmax, frame_len=1200, stride=480, n_frames=F, window=dw)
        assert np.array_equal(n, big[1]) and np.array_equal(s, big[2])
        la.assert_same_bits(f"kmax {kmax}", "cand", c, np.ascontiguousarray(big[0][:, :kmax]))
        assert np.all(big[0][:, kmax:] == 0.0)


def test_degenerate_frames_and_the_reference_call_agree_on_status(vb, pkg):
    """All zeros, one impulse, a NaN sample, an Inf sample (under the Hanning window) and a constant frame (no window: a monotone
    curve): no comparison succeeds, the unvoiced entry alone with VBX_FRAME_OK -- and vbx_pitch_f64 reports the same count and
    status for them."""
    n = 1200
    fr = np.zeros((4, n))
    fr[1, 600] = 1.0
    fr[2, :] = 0.25; fr[2, 5] = np.nan
    fr[3, :] = 0.25; fr[3, 5] = np.inf
    alone = [[0.0, TH]] + [[0.0, 0.0]] * 3
    for frames, dw in ((fr, vb.window(pkg.WINDOW_HANNING, n)), (np.ones((2, n)), None)):
        cand, count, status = vb.pitch_boersma(frames, SR, TH, FMIN, FMAX, kmax=4, window=dw)
        ref, rn, rs = vb.pitch(frames, SR, TH, FMIN, FMAX, kmax=4, window=dw)
        for t in range(frames.shape[0]):
            assert count[t] == 1 and status[t] == 0 and np.array_equal(cand[t], alone), (t, cand[t], count[t], status[t])
            assert rn[t] == count[t] and rs[t] == status[t], (t, rn[t], rs[t])


def _invalid_cases(F, N):
    ok = dict(n_frames=F, frame_len=N, stride=N, sample_rate=SR, fmin=FMIN, fmax=FMAX, kmax=4, x=True, cand=True, count=True)
    for k, v in (("frame_len", 15), ("frame_len", 4097), ("kmax", 0), ("kmax", 64), ("sample_rate", 0.0), ("sample_rate", -1.0),
                 ("sample_rate", float("inf")), ("sample_rate", float("nan")), ("fmin", FMAX), ("fmin", 700.0), ("x", False),
                 ("cand", False), ("count", False), ("stride", 0)):
        yield dict(ok, **{k: v}), f"{k}={v}"


def test_invalid_arguments_write_nothing(vb, pkg):
    """Every VBX_E_INVALID case leaves the outputs' canaries intact and the context usable."""
    F, N = 3, 64
    x = np.sin(np.arange(F * 4097) * 0.05)
    for p, label in _invalid_cases(F, N):
        a = la.Arena(la.DeviceBackend(vb), label)
        a.input("x", x)
        a.output("cand", np.float64, F, 2 * 64)
        a.output("count", np.int32, F, 1)
        a.output("status", np.int32, F, 1)
        a.place()
        rc = vb.L.vbx_pitch_boersma_f64(vb.ctx, a["x"] if p["x"] else None, p["n_frames"], p["frame_len"], p["stride"], None,
                                        p["sample_rate"], TH, p["fmin"], p["fmax"], p["kmax"], a["cand"] if p["cand"] else None,
                                        a["count"] if p["count"] else None, a["status"])
        assert rc == -1, (label, rc)                           # VBX_E_INVALID
        outs = a.finish()
        for nm in ("cand", "count", "status"):
            assert la.unwritten(outs[nm]).shape[0] == outs[nm].size, (label, nm)
    assert vb.L.vbx_pitch_boersma_f64(vb.ctx, None, 0, N, N, None, SR, TH, FMIN, FMAX, 4, None, None, None) == 0    # an empty batch
    cand, count, status = vb.pitch_boersma(x[:F * N].reshape(F, N), SR, TH, FMIN, 30000.0, kmax=4)                 # still usable
    assert np.all(status == 0) and np.all(count >= 1)


def test_lists_go_straight_into_the_pitch_path(vb, pkg, signals):
    """vbx_pitch_boersma_f64 -> vbx_frame_peak_f64 -> vbx_pitch_path_f64: the contour is tests/pitch_path_model.py's on the same
    lists, bit for bit (the path's existing contract on new input)."""
    x, sr = signals["voiced"]
    F, N, hop, kmax = 70, 1200, 480, 15
    x = x[:(F - 1) * hop + N]
    dw = vb.window(pkg.WINDOW_HANNING, N)
    cand, count, status = vb.pitch_boersma(x, sr, TH, FMIN, FMAX, kmax=kmax, frame_len=N, stride=hop, n_frames=F, window=dw)
    peak = vb.frame_peak(x, frame_len=N, stride=hop, n_frames=F)
    params = pkg.PitchPathParams.make(time_step=hop / sr)
    path, index = vb.pitch_path(cand, count, status, peak, params=params)
    p = dict(PM.DEFAULTS, time_step=hop / sr)
    tab = PM.frame_table(cand, count, status, peak, None, p)
    mp, mi = PM.outputs(tab, PM.path_states(tab, None))
    assert np.array_equal(mi, index)
    assert np.array_equal(mp.view(np.int64), path.view(np.int64))
    assert np.mean(index >= 0) > 0.9                            # the stretch is voiced


def test_zz_report():
    print("\npitch_boersma report:", json.dumps({k: v for k, v in REPORT.items() if k != "cases"}))
    out = os.environ.get("VBX_TEST_REPORT_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "pitch_boersma_report.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)
