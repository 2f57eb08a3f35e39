"""tests/analyze_reference.py on the CPU: the top-candidate rule on hand-made cases, the frame loop against direct oracle calls,
and the sweep's grid itself -- is it fit to judge a kernel with?  The oracle against ITSELF on every frame multiplied by
1 + 1e-13 cos(i) (a change far below anything a kernel's summation order does) must give equal statuses, equal candidate counts
and classify_top == "ok" on every frame of every (shape, setting): the inputs themselves never need the tie allowance, so any
allowance tests/test_gpu_analyze_params.py consumes is the kernel's doing.  (The full 48 frames per case were run once, 6,864
frame pairs: 0 swaps, 0 bad, 0 status or count differences; 16 of the 48 are kept here, about 80 s on one core.)"""
import numpy as np
import pytest

import analyze_reference as ar
import __graft_entry__ as g


@pytest.fixture(scope="module")
def synth():
    import importlib
    g.load_package()
    return importlib.import_module(g.PKG_NAME + ".synth")


def test_classify_top_each_answer():
    ec = np.array([[150.0, 0.9000], [75.0, 0.8995], [0.0, 0.2]])
    # ok: inside 1e-4 relative Hz and 1e-4 strength; the edge of each on either side
    assert ar.classify_top((150.0, 0.9), ec, 3) == "ok"
    assert ar.classify_top((150.0 * (1 + 0.9e-4), 0.9 - 0.9e-4), ec, 3) == "ok"
    assert ar.classify_top((150.0 * (1 + 1.1e-4), 0.9), ec, 3) == "bad"
    assert ar.classify_top((150.0, 0.9 + 1.1e-4), ec, 3) == "bad"
    # swap: the runner-up, and the oracle's two best closer than 1e-3
    assert ar.classify_top((75.0, 0.8995), ec, 3) == "swap"
    assert ar.classify_top((75.0, 0.8995 + 0.9e-3), ec, 3) == "swap"
    assert ar.classify_top((75.0, 0.8995 + 1.1e-3), ec, 3) == "bad"                  # not the runner-up's strength
    assert ar.classify_top((0.0, 0.2), ec, 3) == "bad"                               # the third candidate is never a tie swap
    wide = np.array([[150.0, 0.9], [75.0, 0.8985], [0.0, 0.2]])
    assert ar.classify_top((75.0, 0.8985), wide, 3) == "bad"                         # runner-up, but the gap is 1.5e-3
    assert ar.classify_top((75.0, 0.8995), ec[:1], 1) == "bad"                       # the oracle has one candidate: nothing to swap with
    # voiced / unvoiced: a swap only inside a 1e-4 tie
    tie = np.array([[150.0, 0.20005], [0.0, 0.2]])
    assert ar.classify_top((0.0, 0.2), tie, 2) == "swap"
    near = np.array([[150.0, 0.2005], [0.0, 0.2]])
    assert ar.classify_top((0.0, 0.2), near, 2) == "vuv_outside"
    assert ar.classify_top((150.0, 0.2005), np.array([[0.0, 0.2009], [150.0, 0.2005]]), 2) == "vuv_outside"
    assert ar.classify_top((150.0, 0.2005), near, 2) == "ok"
    # an unvoiced oracle top (0 Hz): the relative frequency tolerance is zero wide
    unv = np.array([[0.0, 0.2], [150.0, 0.1]])
    assert ar.classify_top((0.0, 0.2), unv, 2) == "ok"
    assert ar.classify_top((1e-9, 0.2), unv, 2) == "bad"
    assert ar.classify_top((float("nan"), 0.2), unv, 2) == "bad" and ar.classify_top((0.0, float("nan")), unv, 2) == "bad"
    assert ar.tie_gap(ec, 3) == pytest.approx(5e-4) and ar.tie_gap(ec[:1], 1) == np.inf


def test_oracle_records_is_the_frame_loop(oracle, synth):
    """Arbitrary parameters, a subset of frames, parts skipped: the rows are what direct oracle calls on those frames give, and the
    formant estimates are carried from frame to frame and reset where a segment starts."""
    n, hop, sr = 400, 160, 16000.0
    x = synth.synth_speech(20 * hop + n, sample_offset=int(2 * sr), sample_rate=sr)
    est0 = np.array([[320.0, 1.0], [1440.0, 1.0], [2760.0, 1.0]])
    frames = list(range(12))
    rec, st, top2, cnt = ar.oracle_records(oracle, x, n, hop, frames, sr, (0.3, 80.0, 500.0), 10, 8, est0, (9, 50.0, 6000.0), {0, 5})
    cols = ar.record_columns(3, 10, 8, (9, 50.0, 6000.0))
    assert cols == {"pitch": (0, 2), "formants": (2, 6), "mfcc": (8, 9), "lpc": (17, 11), "_width": (28, 0)}
    assert rec.shape == (12, 28) and st.shape == (3, 12) and top2.shape == (12, 2, 2)
    w = oracle.window("hanning", n)
    est = est0.copy()
    for t in frames:
        fr = x[t * hop:t * hop + n]
        s, c, k = oracle.pitch(fr * w, sr, 0.3, 80.0, 500.0)
        assert st[0, t] == s and cnt[t] == k and np.array_equal(top2[t, :min(k, 2)], c[:2]) and np.array_equal(rec[t, 0:2], c[0])
        if t in (0, 5):
            est = est0.copy()
        s, est, _, _ = oracle.find_formants(fr, sr, 8, est)
        assert st[1, t] == s and np.array_equal(rec[t, 2:8], est.reshape(-1))
        s, m = oracle.mfcc(fr * w, 9, 50.0, 6000.0, sr)
        assert st[2, t] == s and np.array_equal(rec[t, 8:17], m)
        assert np.array_equal(rec[t, 17:28], oracle.lpc(oracle.autocorrelate(fr * w, 11), 10))
    assert np.count_nonzero(rec[:, 0]) >= 3                                          # voiced frames among them
    # a subset, out of order, pitch only: the same rows
    r2, s2, t2, c2 = ar.oracle_records(oracle, x, n, hop, [7, 2, 11], sr, (0.3, 80.0, 500.0), 0, 0, None, None, None)
    assert r2.shape == (3, 2) and np.array_equal(r2, rec[[7, 2, 11], 0:2]) and np.array_equal(t2, top2[[7, 2, 11]])
    assert np.array_equal(s2[0], st[0, [7, 2, 11]]) and not s2[1:].any() and np.array_equal(c2, cnt[[7, 2, 11]])
    # no pitch: the pair stays zero, the other columns do not move
    r3, s3, _, _ = ar.oracle_records(oracle, x, n, hop, frames, sr, None, 10, 8, est0, (9, 50.0, 6000.0), {0, 5})
    assert not r3[:, 0:2].any() and np.array_equal(r3[:, 2:], rec[:, 2:]) and np.array_equal(s3[1:], st[1:])


def test_sweep_tables_are_consistent():
    assert len(ar.SHAPES) == 13 and len(set(ar.SHAPES)) == 13
    for n, hop, sr in ar.SHAPES:
        s = ar.settings(n, sr)
        assert len(s) == len(ar.SETTING_NAMES) == 11
        assert ar.DEFAULT_PITCH not in s                                 # the sweep is everything BUT the setting the suite already had
        stride = ar.sweep_stride(n, sr)
        assert stride >= 1 and (ar.SWEEP_FRAMES - 1) * stride + n <= ar.sweep_samples(n, sr)[0]
        # the reach 2 ceil(sr / fmin) + 16 of the edge setting: just below the frame
        reach = 2 * int(np.ceil(sr / ar.pitch_edge(n, sr))) + 16
        assert n - 26 <= reach <= n


@pytest.mark.parametrize("n,hop,sr", ar.SHAPES)
def test_the_grid_never_needs_the_tie_allowance(oracle, synth, n, hop, sr):
    ns, off = ar.sweep_samples(n, sr)
    x = synth.synth_speech(ns, sample_offset=off, sample_rate=sr)
    stride = ar.sweep_stride(n, sr)
    frames = list(range(0, ar.SWEEP_FRAMES, 3))                          # 16 of the sweep's 48, over the same five seconds
    y = x.copy()
    tt = np.arange(n)
    xp = np.zeros((len(frames), n))                                      # the perturbed frames, laid end to end
    for i, t in enumerate(frames):
        xp[i] = x[t * stride:t * stride + n] * (1.0 + 1e-13 * np.cos(tt))
    for name, pitch in zip(ar.SETTING_NAMES, ar.settings(n, sr)):
        _, st, top2, cnt = ar.oracle_records(oracle, y, n, stride, frames, sr, pitch, 0, 0, None, None, None)
        pr, pst, _, pcnt = ar.oracle_records(oracle, xp.reshape(-1), n, n, range(len(frames)), sr, pitch, 0, 0, None, None, None)
        assert np.array_equal(st, pst), (name, st[0], pst[0])
        assert np.array_equal(cnt, pcnt), (name, cnt, pcnt)
        verdicts = [ar.classify_top(pr[i, 0:2], top2[i], cnt[i]) for i in range(len(frames)) if st[0, i] == 0]
        assert verdicts.count("ok") == len(verdicts), (name, verdicts)
