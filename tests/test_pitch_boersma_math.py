"""The definition of vbx_pitch_boersma_f64 on the CPU: tests/pitch_boersma_model.py against a long-double evaluation of the
interpolant, against tones of known frequency, on degenerate frames, and the share of frames whose decisions sit within 1e-9 of
flipping on the inputs the GPU tests use (a condition on those inputs, at most 1 %)."""
import importlib.util
import os
import wave

import numpy as np
import pytest

import pitch_boersma_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
TH, FMIN, FMAX = 0.2, 75.0, 600.0


def _synth():
    spec = importlib.util.spec_from_file_location("vbx_synth_host", os.path.join(ROOT, "vox_box.rs_amd", "synth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tone(n, sr, f0, harmonics):
    t = np.arange(n) / sr
    return sum(np.sin(2.0 * np.pi * f0 * h * t) / h for h in range(1, harmonics + 1))


# at least three periods in the frame
TONES = [(1200, 48000.0, 211.7, 1), (1200, 48000.0, 433.1, 1), (1200, 48000.0, 137.3, 7), (1200, 48000.0, 211.7, 7),
         (1024, 44100.0, 211.7, 1), (1024, 44100.0, 433.1, 1), (1024, 44100.0, 311.3, 7), (1024, 44100.0, 211.7, 7)]


@pytest.mark.parametrize("n,sr,f0,harm", TONES)
def test_tones_land_on_f0_not_on_the_integer_lag(n, sr, f0, harm):
    """The top voiced candidate within 1e-4 relative of f0 (BASELINE's Hz tolerance) and at least ten times closer than the integer
    lag sample_rate / k the reference returns."""
    assert f0 * n / sr >= 3.0
    r = M.frame(tone(n, sr, f0, harm) * M.hanning(n), sr, TH, FMIN, FMAX, 4)
    assert r.status == M.FRAME_OK and r.row[0, 0] > 0.0
    k = r.peaks[r.selected[0]]
    err, err_int = abs(r.row[0, 0] - f0) / f0, abs(sr / k - f0) / f0
    print(f"{n} @ {sr}: {f0} Hz x{harm}: {r.row[0, 0]:.5f} Hz rel {err:.2e}; integer lag {k}: rel {err_int:.2e}")
    assert err <= 1e-4
    assert err * 10.0 <= err_int


def test_every_returned_lag_is_a_local_maximum_of_the_long_double_interpolant():
    """S_ld(xmid) >= max(S_ld(k), S_ld(xmid +- 1e-3)) - 1e-9: Brent stops within 2 tol_act ~ 1e-5 lags of a stationary point of a
    band-limited curve with |S''| of a few units, a deficit of order 1e-10."""
    syn = _synth()
    w = M.hanning(1200)
    worst = -1.0
    for off, F, kmax in ((0, 6, 15), (4 * 48000, 2, 8)):
        x = syn.synth_speech((F - 1) * 480 + 1200, off)
        for t in range(F):
            xw = x[t * 480:t * 480 + 1200] * w
            y = M.curve(xw)
            r = M.frame(xw, SR, TH, FMIN, FMAX, kmax, y=y)
            for pos, xm in zip(r.selected, r.xmid):
                if xm == 0.0:
                    continue
                here = M.S_ld(y, xm, M.DEPTH_REFINE)
                k = r.peaks[pos]
                around = max(M.S_ld(y, float(k), M.DEPTH_REFINE), M.S_ld(y, xm - 1e-3, M.DEPTH_REFINE), M.S_ld(y, xm + 1e-3, M.DEPTH_REFINE))
                worst = max(worst, float(around - here))
                assert here >= around - 1e-9, (off, t, k, xm, float(around - here))
                assert abs(xm - r.x0[pos]) <= 1.0
    print("worst deficit", worst)


def test_float64_interpolant_agrees_with_long_double():
    rng = np.random.default_rng(7)
    y = M.curve(tone(1200, SR, 211.7, 7) * M.hanning(1200))
    for x in rng.uniform(80.0, 598.0, 40):
        a, b = M.S(y, x, M.DEPTH_REFINE), float(M.S_ld(y, x, M.DEPTH_REFINE))
        assert abs(a - b) <= 1e-11 * max(1.0, float(np.sum(np.abs(y[:2 * int(x) + 1])))), (x, a, b)
    assert M.S(y, 100.0, 30) == y[100] and M.S(y, 100.0 + 5e-11, 30) == y[100] and M.S(y, 101.0 - 5e-11, 30) == y[101]
    assert M.S(y, -0.25, 30) == y[0]


def test_degenerate_frames():
    """All zeros (the curve is NaN throughout), one impulse, a NaN sample, an Inf sample: no comparison succeeds, the unvoiced entry
    alone with VBX_FRAME_OK.  A constant frame under the Hanning window has peaks like any other frame; without a window its
    curve has none in range."""
    n, w = 1200, M.hanning(1200)
    frames = {"zeros": np.zeros(n), "impulse": np.eye(1, n, 600)[0], "nan": np.r_[np.full(5, 0.25), np.nan, np.full(n - 6, 0.25)],
              "inf": np.r_[np.full(5, 0.25), np.inf, np.full(n - 6, 0.25)]}
    for name, x in frames.items():
        r = M.frame(x * w, SR, TH, FMIN, FMAX, 4)
        assert r.count == 1 and r.status == M.FRAME_OK, name
        assert np.array_equal(r.row, [[0.0, TH], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]), (name, r.row)
    assert np.all(np.isnan(M.curve(np.zeros(n))))
    r = M.frame(np.ones(n), SR, TH, FMIN, FMAX, 4)               # constant, no window: a monotone curve
    assert r.count == 1 and r.status == M.FRAME_OK and np.array_equal(r.row[0], [0.0, TH])
    r = M.frame(np.ones(n) * w, SR, TH, FMIN, FMAX, 4)
    assert r.status == M.FRAME_OK and r.count >= 1


def test_a_nan_strength_is_reported_not_dropped():
    """A curve with a NaN inside the reach of a peak's sums: the entry's s1 is NaN, it is selected first, and the frame reports
    VBX_FRAME_ERR_NAN with a zero row and count 0."""
    y = M.curve(tone(1200, SR, 211.7, 1) * M.hanning(1200))
    y = y.copy()
    y[240] = np.nan                                              # 13 lags from the peak at 227: inside S_30, outside the peak test
    r = M.frame(None, SR, TH, FMIN, FMAX, 2, y=y)
    assert r.status == M.FRAME_ERR_NAN and r.count == 0 and np.all(r.row == 0.0)


def test_selection_is_by_first_pass_strength_and_rows_are_not_prefixes():
    syn = _synth()
    x = syn.synth_speech(1200, 4 * 48000 + 4800) * M.hanning(1200)          # noise: far more candidates than kmax
    y = M.curve(x)
    big = M.frame(x, SR, TH, FMIN, FMAX, 63, y=y)
    assert big.count > 63
    for kmax in (1, 2, 4):
        r = M.frame(x, SR, TH, FMIN, FMAX, kmax, y=y)
        assert r.count == big.count
        s1 = np.array([M._key(s) for s in r.s1])
        want = sorted(np.lexsort((np.arange(s1.size), -s1))[:kmax])
        assert sorted(r.selected) == want
        assert np.all(np.diff(r.row[:, 1]) <= 0.0)
    # kmax >= count: the whole list, whatever kmax
    v = syn.synth_speech(1200, 0) * M.hanning(1200)
    a, b = M.frame(v, SR, TH, FMIN, FMAX, 40), M.frame(v, SR, TH, FMIN, FMAX, 63)
    assert a.count <= 40 and np.array_equal(a.row, b.row[:40]) and np.all(b.row[40:] == 0.0)


def _wav(path):
    with wave.open(path, "rb") as w:
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        return pcm.astype(np.float64) / 32767.0, float(w.getframerate())


def test_flagged_share_on_the_gpu_tests_inputs():
    """At most 1 % of the frames of every input tests/test_gpu_pitch_boersma.py uses may have a decision within 1e-9 of flipping (a
    condition on the inputs: one that exceeds it is replaced, the cap stays).  The host generator stands in for the device's
    (they agree to rounding)."""
    syn = _synth()
    wav, wsr = _wav(os.path.join(ROOT, "tests", "golden", "sample-two_vowels.wav"))
    inputs = [("voiced", syn.synth_speech(62 * 480 + 1200, 0), SR, 1200, 480, 63, 15, FMAX),
              ("noise", syn.synth_speech(30 * 480 + 1200, 4 * 48000 - 2400), SR, 1200, 480, 31, 4, FMAX),
              ("voiced-64", syn.synth_speech(257 * 64, 0), SR, 64, 64, 257, 2, 30000.0),
              ("vowels", wav, wsr, 1024, 512, 33, 15, FMAX)]
    for name, x, sr, n, hop, F, kmax, fmax in inputs:
        assert x.size >= (F - 1) * hop + n, name
        w = M.hanning(n) if name != "voiced-64" else None
        _, count, _, res = M.pitch_boersma(x, F, n, hop, w, sr, TH, FMIN, fmax, kmax)
        flagged = sum(r.flagged for r in res)
        print(f"{name}: {flagged} of {F} frames flagged, mean count {count.mean():.1f}, max {count.max()}")
        assert flagged <= 0.01 * F, (name, flagged, F)
