"""VBX_LPC_POLICY_REFERENCE: every autocorrelation and LPC row the library computes from frames is BIT FOR BIT the row the
crate computes -- the sequential lag fold of src/periodic.rs:276-289 and the recursion of src/spectrum.rs:63-84 in IEEE f64
without contraction (oracle/vbx_oracle.c states both line by line).  No tolerance and no arbiter: NaN positions are compared,
then the bits of everything else.  The default policy's rows are untouched (tests/test_gpu_lpc_exact.py, test_gpu_soak.py);
under REFERENCE every other column of an analyze record is the default policy's, bit for bit."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR48, N48, H48 = 48000.0, 1200, 480


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


def _rows_differing(a, b):
    """Indices of the rows of a and b that are not bit for bit the same (NaN positions compared separately)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    bits = np.where(na | nb, 0, a.view(np.int64)) != np.where(na | nb, 0, b.view(np.int64))
    return np.nonzero(np.any(bits | (na != nb), axis=1))[0]


def _parity_metric(a, b):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6 * np.max(np.abs(b), axis=1, keepdims=True)), axis=1)


@pytest.fixture(scope="module")
def ref(pkg):
    v = pkg.VoxBox(0, lpc_policy=pkg.LPC_POLICY_REFERENCE)
    yield v
    v.close()


@pytest.fixture(scope="module")
def speech_pcm(golden_dir):
    with wave.open(os.path.join(golden_dir, "sample-two_vowels.wav"), "rb") as w:
        sr = float(w.getframerate())
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return sr, pcm


def _speech(pkg, pcm, ns):
    import torch
    from importlib import import_module
    syn = import_module(pkg.__name__ + ".synth")
    return syn.speech_recording(torch, "cpu", pcm, ns).numpy()      # as test_soak_real_speech_44k builds it


# ---- 1. shapes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,lags", [(512, 13), (512, 1), (16, 16), (100, 7), (1200, 13), (1200, 1200),
                                    (333, 333), (2048, 17), (4096, 40), (640, 321), (64, 64), (5, 5),
                                    (1300, 1290), (4096, 4096), (1280, 257),
                                    (512, 64), (512, 511), (1024, 1024), (1103, 1103), (1200, 65), (2047, 1001), (2048, 2048),
                                    (3000, 64), (640, 63), (1024, 18), (2048, 40),
                                    (4097, 13), (70001, 13), (70001, 70)])
def test_autocorrelate_is_the_crates_fold(ref, oracle, n, lags):
    rng = np.random.default_rng(n * 1000 + lags)
    x = rng.uniform(-1, 1, (9 if n <= 4096 else 3, n))       # rectangular frames: x[0] != 0 exercises the Q1 seed
    got = ref.autocorrelate(x, lags)
    exp = np.stack([oracle.autocorrelate(f, lags) for f in x])
    assert _bits_equal(got, exp), _rows_differing(got, exp)


@pytest.mark.parametrize("n,hop,lags", [(1200, 480, 13), (1200, 480, 1200), (480, 160, 100)])
def test_autocorrelate_strided_windowed(ref, oracle, pkg, n, hop, lags):
    audio = ref.synth_speech(40 * hop + n, sample_offset=48000).numpy()
    F = pkg.frame_count(audio.size, n, hop)
    w = pkg.window_table(pkg.WINDOW_HANNING, n)
    got = ref.autocorrelate(audio, lags, frame_len=n, stride=hop, window=ref.to_device(w))
    exp = np.stack([oracle.autocorrelate(audio[t * hop:t * hop + n] * w, lags) for t in range(F)])
    assert _bits_equal(got, exp), _rows_differing(got, exp)


@pytest.mark.parametrize("p", [1, 8, 12, 13, 16, 31, 46, 62])
def test_autocorr_lpc_orders_and_lengths(ref, oracle, pkg, p):
    rng = np.random.default_rng(p)
    for n in (30, 63, 100, 512, 1103, 4096, 5000):
        if n < p + 1:
            continue
        x = rng.uniform(-1, 1, (7, n))
        w = pkg.window_table(pkg.WINDOW_HANNING, n)
        for window in (None, w):
            xw = x if window is None else x * w[None, :]
            for normalize in (False, True):
                r, a = ref.autocorr_lpc(x, p, normalize=normalize, window=None if window is None else ref.to_device(window))
                er = np.stack([oracle.autocorrelate(f, p + 1) for f in xw])
                if normalize:
                    er = np.stack([oracle.normalize(row) for row in er])
                ea = np.stack([oracle.lpc(row, p) for row in er])
                assert _bits_equal(r, er), (n, normalize, window is None, _rows_differing(r, er))
                assert _bits_equal(a, ea), (n, normalize, window is None, _rows_differing(a, ea))


@pytest.mark.parametrize("p", [1, 12, 13, 40])
@pytest.mark.parametrize("F", [0, 1, 3, 5, 7, 9, 17, 33])
def test_batch_sizes(ref, oracle, pkg, p, F):
    """0, 1 and sizes that are not multiples of the frames per wavefront (8 at order 1, 4 at 12 / 13, 1 at 40)."""
    n = 700
    if F == 0:
        assert ref.L.vbx_autocorr_lpc_f64(ref.ctx, None, 0, n, n, None, p, 0, None, None) == 0
        assert ref.L.vbx_autocorrelate_f64(ref.ctx, None, 0, n, n, None, p + 1, None) == 0
        return
    x = np.random.default_rng(F * 100 + p).uniform(-1, 1, (F, n))
    r, a = ref.autocorr_lpc(x, p)
    er = np.stack([oracle.autocorrelate(f, p + 1) for f in x])
    assert _bits_equal(r, er) and _bits_equal(a, np.stack([oracle.lpc(row, p) for row in er]))


def test_lpc_rows_entry_points(ref, oracle, pkg):
    """vbx_lpc_f64 / vbx_lpc_mut_f64 under REFERENCE: the recursion operation for operation (rows of real lag sums,
    orders up to VBX_MAX_LPC_ORDER, strided input)."""
    audio = ref.synth_speech(64 * 512, sample_offset=5 * 48000).numpy().reshape(64, 512)
    w = pkg.window_table(pkg.WINDOW_HANNING, 512)
    rows = np.stack([oracle.autocorrelate(f * w, 63) for f in audio])
    for p in (1, 2, 12, 13, 31, 62):
        exp = np.stack([oracle.lpc(r, p) for r in rows])
        assert _bits_equal(np.stack([_levinson_kc(r, p) for r in rows])[:, -1], exp[:, -1])     # (the restatement below)
        got = ref.lpc(rows, p)                                                        # r_stride 63 > p + 1
        assert _bits_equal(got, exp), (p, _rows_differing(got, exp))
        ac, kc = ref.lpc_mut(rows, p)
        ekc = np.stack([_levinson_kc(r, p) for r in rows])
        assert _bits_equal(ac, exp), p
        assert _bits_equal(kc, ekc), (p, _rows_differing(kc, ekc))


def _levinson_kc(r, p):
    """The reflection coefficients lpc_mut leaves in `kc` (src/spectrum.rs:63-84), restated in Python floats (IEEE f64, no
    contraction: the oracle's operations one by one); the coefficients it yields are checked against the oracle's as well."""
    ac, kc, err = [1.0] + [0.0] * p, [0.0] * p, float(r[0])
    for i in range(1, p + 1):
        acc = float(r[i])
        for j in range(1, i):
            acc = acc + ac[j] * float(r[i - j])
        kc[i - 1] = -acc / err
        ac[i] = kc[i - 1]
        tmp = list(ac)
        for j in range(1, i):
            ac[j] = ac[j] + kc[i - 1] * tmp[i - j]
        err = err * (1.0 - kc[i - 1] * kc[i - 1])
    return np.array(kc)


# ---- 2. the rows that differ today ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,hop", [(1103, 441), (1024, 512)])
def test_real_speech_rows_are_the_crates(pkg, oracle, ref, speech_pcm, n, hop):
    F, order = 20000, 13
    sr, pcm = speech_pcm
    audio = _speech(pkg, pcm, (F - 1) * hop + n)
    params = pkg.AnalysisParams.make(sr, pitch=(0.2, 75.0, 600.0), lpc_order=order, formant_order=0, mfcc=(13, 100.0, 8000.0))
    l0, ln = params.columns()["lpc"]
    s = oracle.soak(audio, n, hop, 0, F, order, sr, oracle.SOAK_LPC)
    ad = ref.to_device(audio)
    rec, _ = ref.analyze_frames(ad, params, frame_len=n, stride=hop, n_frames=F)
    assert ref.last_lpc_exact_count() == -1
    bad = _rows_differing(rec[:, l0:l0 + ln], s["a"])
    assert bad.size == 0, (bad.size, bad[:8])
    with pkg.VoxBox(0, lpc_policy=pkg.LPC_POLICY_EXACT) as v:
        d = v.to_device(audio)
        rd, _ = v.analyze_frames(d, params, frame_len=n, stride=hop, n_frames=F)
    beyond = int(np.sum(_parity_metric(rd[:, l0:l0 + ln], s["a"]) > 1e-6))
    assert beyond >= 1, "the material does not exercise the ill-conditioned rows"


def test_default_shard_rows_are_the_crates(pkg, oracle, ref):
    F, order = 50000, 12
    ad = ref.synth_speech((F - 1) * H48 + N48, sample_offset=0)
    audio = ad.numpy()
    params = pkg.AnalysisParams.make(SR48, pitch=(0.2, 75.0, 600.0), lpc_order=order, formant_order=0, mfcc=(13, 100.0, 8000.0))
    l0, ln = params.columns()["lpc"]
    rec, _ = ref.analyze_frames(ad, params, frame_len=N48, stride=H48, n_frames=F)
    s = oracle.soak(audio, N48, H48, 0, F, order, SR48, oracle.SOAK_LPC)
    bad = _rows_differing(rec[:, l0:l0 + ln], s["a"])
    assert bad.size == 0, (bad.size, bad[:8])


def test_config2_rows_are_the_crates(pkg, oracle, ref):
    F, order = 20000, 12
    ad = ref.synth_speech(F * 512, sample_offset=0)
    audio = ad.numpy()
    r, a = ref.autocorr_lpc(ad, order, frame_len=512, stride=512, n_frames=F, window=ref.window(pkg.WINDOW_HANNING, 512))
    s = oracle.soak(audio, 512, 512, 0, F, order, SR48, oracle.SOAK_LPC)
    assert _rows_differing(r, s["r"]).size == 0
    bad = _rows_differing(a, s["a"])
    assert bad.size == 0, (bad.size, bad[:8])


# ---- 3. pcm16 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,hop,order,sr", [(1200, 480, 12, 48000.0), (1103, 441, 13, 44100.0)])
def test_pcm16_rows_are_the_crates(pkg, oracle, ref, n, hop, order, sr):
    """1200 / 480 at order 12 reads the PCM directly (the fused kernel); 1103 / 441 at order 13 is widened first."""
    F = 3000
    rng = np.random.default_rng(n)
    t = np.arange((F - 1) * hop + n)
    sig = 9000 * np.sin(2 * np.pi * 180 * t / sr) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t / sr)) + rng.normal(0, 300, t.size)
    pcm = np.clip(np.round(sig), -32768, 32767).astype(np.int16)
    params = pkg.AnalysisParams.make(sr, pitch=(0.2, 75.0, 600.0), lpc_order=order, formant_order=0, mfcc=(13, 100.0, 8000.0))
    l0, ln = params.columns()["lpc"]
    rec, _ = ref.analyze_frames_pcm16(pcm, params, frame_len=n, stride=hop)
    s = oracle.soak(pcm.astype(np.float64) / 32767.0, n, hop, 0, F, order, sr, oracle.SOAK_LPC)
    bad = _rows_differing(rec[:, l0:l0 + ln], s["a"])
    assert bad.size == 0, (bad.size, bad[:8])


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,hop,order,form", [(1200, 480, 12, "f64"), (1200, 480, 12, "pcm16"), (1103, 441, 13, "f64"),
                                              (1024, 512, 13, "pcm16"), (5000, 2000, 12, "f64")])
def test_other_columns_do_not_move(pkg, n, hop, order, form):
    F = 600 if n <= 4096 else 40
    sr = 48000.0
    with pkg.VoxBox(0) as d, pkg.VoxBox(0, lpc_policy=pkg.LPC_POLICY_REFERENCE) as r:
        audio = d.synth_speech((F - 1) * hop + n, sample_offset=2 * 48000).numpy()
        est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
        params = pkg.AnalysisParams.make(sr, pitch=(0.2, 75.0, 600.0), lpc_order=order, formant_order=order, est_init=est0,
                                         mfcc=(13, 100.0, 8000.0))
        l0, ln = params.columns()["lpc"]
        if form == "pcm16":
            pcm = np.clip(np.round(audio * 32767.0), -32768, 32767).astype(np.int16)
            run = lambda v: v.analyze_frames_pcm16(pcm, params, frame_len=n, stride=hop)
        else:
            run = lambda v: v.analyze_frames(audio, params, frame_len=n, stride=hop)
        rd, sd = run(d)
        rr, sr_ = run(r)
    keep = np.ones(rd.shape[1], dtype=bool)
    keep[l0:l0 + ln] = False
    assert _bits_equal(rr[:, keep], rd[:, keep])
    assert np.array_equal(sr_, sd)
    assert not _bits_equal(rr[:, l0:l0 + ln], rd[:, l0:l0 + ln]) or n == 5000     # (a 5000-sample frame has no probe to differ by)


def test_toggling_back_reproduces_a_fresh_context(pkg):
    F, n, hop = 400, 1103, 441
    with pkg.VoxBox(0) as fresh, pkg.VoxBox(0) as t:
        audio = fresh.synth_speech((F - 1) * hop + n, sample_offset=48000).numpy()
        params = pkg.AnalysisParams.make(44100.0, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=0, mfcc=(13, 100.0, 8000.0))
        w = fresh.window(pkg.WINDOW_HANNING, n)
        want = fresh.analyze_frames(audio, params, frame_len=n, stride=hop)[0], fresh.autocorr_lpc(audio, 13, frame_len=n, stride=hop, window=w)
        t.lpc_policy = pkg.LPC_POLICY_REFERENCE
        t.analyze_frames(audio, params, frame_len=n, stride=hop)
        t.autocorr_lpc(audio, 13, frame_len=n, stride=hop, window=t.window(pkg.WINDOW_HANNING, n))
        t.lpc_policy = pkg.LPC_POLICY_EXACT
        got = t.analyze_frames(audio, params, frame_len=n, stride=hop)[0], t.autocorr_lpc(audio, 13, frame_len=n, stride=hop,
                                                                                          window=t.window(pkg.WINDOW_HANNING, n))
    assert _bits_equal(got[0], want[0])
    assert _bits_equal(got[1][0], want[1][0]) and _bits_equal(got[1][1], want[1][1])


def test_policy_initial_value_set_and_errors(pkg, monkeypatch):
    with pkg.VoxBox(0) as v:
        assert v.lpc_policy == pkg.LPC_POLICY_EXACT
        assert v.L.vbx_ctx_set_lpc_policy(v.ctx, 3) == -1 and v.L.vbx_ctx_set_lpc_policy(v.ctx, -1) == -1     # VBX_E_INVALID
        assert v.lpc_policy == pkg.LPC_POLICY_EXACT
        n = C.c_int(7)
        assert v.L.vbx_ctx_get_lpc_policy(None, C.byref(n)) == -1
    monkeypatch.setenv("VBX_LPC_EXACT", "0")
    with pkg.VoxBox(0) as v:
        assert v.lpc_policy == pkg.LPC_POLICY_PLAIN
        v.lpc_policy = pkg.LPC_POLICY_REFERENCE
        assert v.lpc_policy == pkg.LPC_POLICY_REFERENCE
    with pkg.VoxBox(0, lpc_policy=pkg.LPC_POLICY_EXACT) as v:
        assert v.lpc_policy == pkg.LPC_POLICY_EXACT
    monkeypatch.delenv("VBX_LPC_EXACT")
    with pytest.raises(pkg.VoxBoxError):
        pkg.VoxBox(0, lpc_policy=5)


def test_exact_count_is_minus_one_after_a_reference_call(pkg):
    F, n, hop = 300, 1200, 480
    with pkg.VoxBox(0) as v:
        audio = v.synth_speech((F - 1) * hop + n, sample_offset=0).numpy()
        params = pkg.AnalysisParams.make(SR48, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=0, mfcc=(13, 100.0, 8000.0))
        v.analyze_frames(audio, params, frame_len=n, stride=hop)
        assert v.last_lpc_exact_count() >= 0
        v.lpc_policy = pkg.LPC_POLICY_REFERENCE
        v.analyze_frames(audio, params, frame_len=n, stride=hop)
        assert v.last_lpc_exact_count() == -1
        v.autocorr_lpc(audio, 12, frame_len=n, stride=hop, window=v.window(pkg.WINDOW_HANNING, n))
        assert v.last_lpc_exact_count() == -1
        v.lpc_policy = pkg.LPC_POLICY_EXACT
        v.autocorr_lpc(audio, 12, frame_len=n, stride=hop, window=v.window(pkg.WINDOW_HANNING, n))
        assert v.last_lpc_exact_count() >= 0
        v.pitch(audio, SR48, 0.2, 75.0, 600.0, kmax=1, frame_len=n, stride=hop)       # a call without LPC rows: no stale count
        assert v.last_lpc_exact_count() == -1
        v.autocorr_lpc(audio, 12, frame_len=n, stride=hop, window=v.window(pkg.WINDOW_HANNING, n))
        assert v.last_lpc_exact_count() >= 0
        v.mfcc(audio, 13, (100.0, 8000.0), SR48, frame_len=n, stride=hop, window=v.window(pkg.WINDOW_HANNING, n))
        assert v.last_lpc_exact_count() == -1


# ---- 5. degenerate rows -------------------------------------------------------------------------------------------------

def _degenerate_frames(n):
    t = np.arange(n)
    rng = np.random.default_rng(n)
    nan = rng.uniform(-1, 1, n)
    nan[n // 3] = np.nan
    nan0 = rng.uniform(-1, 1, n)
    nan0[0] = np.nan
    return np.stack([np.zeros(n), np.full(n, 0.25), np.full(n, -1.0), np.sin(2 * np.pi * 7 * t / n),
                     np.cos(2 * np.pi * 50.5 * t / n), rng.uniform(-1, 1, n) + 3.0, nan, nan0,
                     np.concatenate([[1.0], np.zeros(n - 1)]), np.concatenate([np.zeros(n - 1), [1.0]])])


@pytest.mark.parametrize("n", [64, 1200, 4500])
@pytest.mark.parametrize("p", [12, 13])
def test_degenerate_rows(ref, oracle, pkg, n, p):
    x = _degenerate_frames(n)
    for window in (None, pkg.window_table(pkg.WINDOW_HANNING, n)):
        xw = x if window is None else x * window[None, :]
        for normalize in (False, True):
            r, a = ref.autocorr_lpc(x, p, normalize=normalize, window=None if window is None else ref.to_device(window))
            er = np.stack([oracle.autocorrelate(f, p + 1) for f in xw])
            if normalize:
                er = np.stack([oracle.normalize(row) for row in er])
            ea = np.stack([oracle.lpc(row, p) for row in er])
            assert _bits_equal(r, er), (normalize, _rows_differing(r, er))
            assert _bits_equal(a, ea), (normalize, _rows_differing(a, ea))
    assert np.any(np.isnan(a[0])) or np.any(np.isinf(a[0]))                            # the silent frame: err = 0
