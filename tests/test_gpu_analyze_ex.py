"""vbx_analyze_frames_ex_f64 / _pcm16 and vbx_find_formants_resampled_f64 on a real MI355X: the frame loop of
examples/formant_extraction/src/main.rs:72-88 -- find_formants at a resample_ratio, the frame's RMS as the record's last column --
from one call.  "The sequence" below is the same work taken apart, from the same build: the plain or tracked call with
formant_order = 0 for the other columns, vbx_resample_linear_f64 into a dense batch and vbx_find_formants_f64 on it, vbx_rms_f64.
The call equals the sequence BIT FOR BIT at every shape; the sequence's parts are held to the oracle by the existing tests, and
the call itself is held to it here."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import layout_arena as la

pytestmark = pytest.mark.gpu

SR = 48000.0
OFFSET = 3 * 48000 + 12345
N_AUDIO = 6 * 48000
E_INVALID = -1
# (frame_len, hop, ratio, order, frames, takes the one-pass lag kernels): every path of the resampled loaders and the dense fallback
SHAPES = [
    (500, 100, 10000.0 / 44100.0, 13, 700, False),      # the example: m = 114, the direct kernel, 4 frames per wavefront
    (1200, 480, 10000.0 / 48000.0, 12, 500, False),     # m = 250: the direct kernel (no one-pass form below 256 samples)
    (1200, 480, 0.25, 12, 500, True),                   # m = 300: the lag kernel, 8 samples per lane
    (1103, 441, 10000.0 / 44100.0, 13, 500, False),     # m = 251: odd, a lane straddles the resampled frame's end
    (2048, 1024, 0.5, 16, 250, True),                   # m = 1024: 16 samples per lane
    (2400, 480, 0.5, 12, 500, True),                    # m = 1200: 20 samples per lane
    (200, 100, 1.5, 8, 1000, True),                     # m = 300: upsampling, the last outputs read past the source frame
    (1200, 480, 0.25, 5, 300, False),                   # orders off the one-pass list: the direct kernel at m = 300 ...
    (1200, 480, 0.25, 20, 300, False),                  # ... and with 32 lanes per frame
    (4096, 2048, 0.5, 12, 120, True),                   # m = 2048: the dense fallback (the segmented lag kernel)
    (5000, 2500, 0.2, 12, 100, True),                   # a source frame beyond VBX_MAX_FRAME_LEN: the dense fallback
]


def _i64(a):
    return np.ascontiguousarray(a).view(np.int64)


def _est0(pkg):
    return np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])


@pytest.fixture(scope="module")
def audio(vb):
    d = vb.synth_speech(N_AUDIO, sample_offset=OFFSET)
    h = d.numpy()
    d.free()
    return h


def _read_pcm16(path):
    with wave.open(path, "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").copy(), float(w.getframerate())


def _params(pkg, order, sr=SR, **kw):
    return pkg.AnalysisParams.make(sr, formant_order=order, est_init=_est0(pkg), **kw)


def _width(vb, params, ext):
    return int(vb.L.vbx_record_doubles_ex(C.byref(params), None if ext is None else C.byref(ext)))


def _formant_rate(params, ext):
    ratio = ext.formant_resample_ratio if ext is not None else 0.0
    if ext is not None and ext.formant_sample_rate != 0.0:
        return ext.formant_sample_rate
    return params.sample_rate * ratio if ratio not in (0.0, 1.0) else params.sample_rate


def _sequence(vb, pkg, x_d, params, ext, N, H, F, seg=None, track=None):
    """The parts taken separately.  Returns (records [F, width], status3, tracked lists or None, the Burg guard's count)."""
    rest = pkg.AnalysisParams.from_buffer_copy(params)
    rest.formant_order, rest.n_est = 0, 0
    lists = None
    if track is None:
        rec0, st = vb.analyze_frames(x_d, rest, seg_start=seg, frame_len=N, stride=H, n_frames=F)
    else:
        rec0, st, *lists = vb.analyze_frames_tracked(x_d, rest, track, seg_start=seg, frame_len=N, stride=H, n_frames=F, lists=True)
    width = _width(vb, params, ext)
    out = np.zeros((F, width))
    cols, cols0 = params.columns(), rest.columns()
    for name, (c0, w) in cols0.items():
        out[:, cols[name][0]:cols[name][0] + w] = rec0[:, c0:c0 + w]
    direct = None
    if params.formant_order:
        ratio = ext.formant_resample_ratio if ext is not None else 0.0
        est = np.array([[params.est_init[i].frequency, params.est_init[i].bandwidth] for i in range(int(params.n_est))])
        rate, p = _formant_rate(params, ext), int(params.formant_order)
        if ratio not in (0.0, 1.0):
            m = int(vb.L.vbx_resampled_len(N, ratio))
            rs = vb.empty((F, m))
            vb.resample_linear(x_d, ratio, frame_len=N, stride=H, n_frames=F, out=rs)
            ff = vb.find_formants(rs, rate, p, est, seg_start=seg, frame_len=m, stride=m, n_frames=F, want=("formants", "status"))
            direct = vb.last_burg_direct_count()
            rs.free()
        else:
            ff = vb.find_formants(x_d, rate, p, est, seg_start=seg, frame_len=N, stride=H, n_frames=F, want=("formants", "status"))
            direct = vb.last_burg_direct_count()
        c0, w = cols["formants"]
        out[:, c0:c0 + w] = ff["formants"].reshape(F, w)
        st[1] = ff["status"]
    if ext is not None and ext.rms:
        out[:, width - 1] = vb.rms(x_d, frame_len=N, stride=H, n_frames=F)
    return out, st, lists, direct


def _ex(vb, x_d, params, ext, N, H, F, seg=None, track=None, pcm=False, lists=False):
    fn = vb.analyze_frames_ex_pcm16 if pcm else vb.analyze_frames_ex
    got = fn(x_d, params, ext, track, seg_start=seg, frame_len=N, stride=H, n_frames=F, lists=lists)
    return (got[0][:, :_width(vb, params, ext)],) + tuple(got[1:])


def _assert_records(label, got, st, want, want_st, params, ext):
    cols = dict(params.columns())
    if ext is not None and ext.rms:
        cols["rms"] = (want.shape[1] - 1, 1)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    for name, (c0, w) in cols.items():
        a, b = _i64(got[:, c0:c0 + w]), _i64(want[:, c0:c0 + w])
        assert np.array_equal(a, b), (label, name, "first differing frame", int(np.argwhere(a != b)[0][0]))
    for row, name in enumerate(("pitch", "formant", "mfcc")):
        assert np.array_equal(st[row], want_st[row]), (label, name + " status", np.nonzero(st[row] != want_st[row])[0][:8])


# ---- 1. bit for bit against the sequence ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,ratio,order,F,one_pass", SHAPES)
def test_the_call_is_the_sequence_bit_for_bit(vb, pkg, audio, N, H, ratio, order, F, one_pass):
    x_d = vb.to_device(audio[:(F - 1) * H + N])
    params = _params(pkg, order)
    ext = pkg.AnalysisExt.make(ratio, rms=True)
    m = int(vb.L.vbx_resampled_len(N, ratio))
    assert m == {500: 114, 1103: 251, 2048: 1024, 2400: 1200, 200: 300, 4096: 2048, 5000: 1000}.get(N, 250 if ratio < 0.25 else 300)
    got, st = _ex(vb, x_d, params, ext, N, H, F)
    direct = vb.last_burg_direct_count()
    want, want_st, _, want_direct = _sequence(vb, pkg, x_d, params, ext, N, H, F)
    x_d.free()
    assert got.shape[1] == 2 + 8 + 13 + 13 + 1
    _assert_records(f"{N}/{H} r {ratio:.4f} p {order}", got, st, want, want_st, params, ext)
    assert direct == want_direct and (direct >= 0) == one_pass, (direct, want_direct)      # the same Burg form as the dense path's
    assert np.all(st[1] == 0) and np.all(np.isfinite(got))


def test_silent_tone_and_nan_frames_take_the_list_form(vb, pkg, audio):
    """m = 300 at order 12 with one silent frame, one pure-tone frame and a NaN sample: the one-pass guard always turns the first
    two away, so the direct recursion's LIST form runs on the resampled view."""
    N, H, ratio, order, F = 1200, 480, 0.25, 12, 300
    sig = audio[:(F - 1) * H + N].copy()
    t_silent, t_tone, t_nan = 40, 120, 200
    sig[t_silent * H:t_silent * H + N] = 0.0
    sig[t_tone * H:t_tone * H + N] = 0.5 * np.sin(2.0 * np.pi * 440.0 * np.arange(N) / SR)
    sig[t_nan * H + N // 2] = np.nan
    x_d = vb.to_device(sig)
    params = _params(pkg, order)
    ext = pkg.AnalysisExt.make(ratio, rms=True)
    got, st = _ex(vb, x_d, params, ext, N, H, F)
    direct = vb.last_burg_direct_count()
    want, want_st, _, want_direct = _sequence(vb, pkg, x_d, params, ext, N, H, F)
    x_d.free()
    _assert_records("special frames", got, st, want, want_st, params, ext)
    assert direct == want_direct and direct > 0, (direct, want_direct)
    assert st[1][t_silent] == pkg.FRAME_ERR_LPC
    for t in np.nonzero(st[1] != 0)[0]:                        # the tracker state passes through a failed frame untouched
        assert t > 0 and np.array_equal(_i64(got[t, 2:10]), _i64(got[t - 1, 2:10])), t
    c_rms = got.shape[1] - 1
    assert got[t_silent, c_rms] == 0.0 and np.isnan(got[t_nan, c_rms]) and abs(got[t_tone, c_rms] - 0.5 / np.sqrt(2.0)) < 1e-3


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------------

def _check_against_oracle(oracle, rec, st, frames, window, pitch_args, rate, ratio, order, est, with_pitch=True):
    """Statuses and counts exact, formants 1e-4 relative, RMS 1e-12 absolute; the top-tie and unstable-frame rules of
    test_gpu_fixtures.test_formant_extraction_example.  Returns (top ties, unstable frames)."""
    ties = unstable = 0
    c_rms = rec.shape[1] - 1
    for t, fr in enumerate(frames):
        if with_pitch:
            es, ec, en = oracle.pitch(fr * window, *pitch_args)
            assert st[0][t] == es == 0, t
            ok = abs(rec[t, 0] - ec[0, 0]) <= 1e-4 * abs(ec[0, 0]) and abs(rec[t, 1] - ec[0, 1]) <= 1e-4
            if not ok:      # only inside a tie of the oracle's own two best strengths
                assert en > 1 and abs(ec[0, 1] - ec[1, 1]) < 1e-4 and abs(rec[t, 0] - ec[1, 0]) <= 1e-4 * abs(ec[1, 0]), (t, rec[t, :2], ec[:2])
                ties += 1
        assert abs(rec[t, c_rms] - oracle.rms(fr)) <= 1e-12, t
        prev = est.copy()
        fs, est = oracle.find_formants_ratio(fr, rate, ratio, order, est)
        assert st[1][t] == fs, t
        got = rec[t, 2:2 + 2 * est.shape[0]].reshape(est.shape)
        if not np.all(np.abs(got - est) <= 1e-4 * np.abs(est)):
            # is the ORACLE's own answer stable under a 1e-13 perturbation of the frame?
            s2, e2 = oracle.find_formants_ratio(fr * (1.0 + 1e-13), rate, ratio, order, prev)
            assert not np.all(np.abs(e2 - est) <= 1e-6 * np.abs(est)), (t, got, est)
            unstable += 1
            est = got.copy()                                   # follow the GPU's track from here (the state is carried)
    return ties, unstable


def test_the_example_on_its_own_recording(vb, oracle, pkg, golden_dir):
    """examples/formant_extraction/src/main.rs:36-88 literally: samples / -65536, bin 500, hop 100, pitch(10000, 0.2, .., 50, 200),
    find_formants(frame, 10000, 10000 / 44100, .., 13, ..) carried over one utterance, the RMS -- one call."""
    pcm, sr = _read_pcm16(os.path.join(golden_dir, "sample-two_vowels.wav"))
    samples = pcm.astype(np.float64) / -65536.0
    N, H, order, new_sr = 500, 100, 13, 10000.0
    ratio = new_sr / sr
    F = pkg.frame_count(samples.size, N, H)
    assert F == 1245
    params = pkg.AnalysisParams.make(new_sr, pitch=(0.2, 50.0, 200.0), lpc_order=0, formant_order=order, est_init=_est0(pkg), mfcc=None)
    ext = pkg.AnalysisExt.make(ratio, formant_sample_rate=new_sr, rms=True)
    x_d = vb.to_device(samples)
    rec, st = _ex(vb, x_d, params, ext, N, H, F)
    x_d.free()
    assert rec.shape == (F, 2 + 8 + 1) and np.all(st[2] == 0)
    frames = [samples[t * H:t * H + N] for t in range(F)]
    ties, unstable = _check_against_oracle(oracle, rec, st, frames, oracle.window("hanning", N), (new_sr, 0.2, 50.0, 200.0), new_sr,
                                           ratio, order, _est0(pkg))
    print(f"example: frames {F}, pitch top ties {ties}, oracle-unstable frames {unstable}")
    assert ties <= 1 and unstable <= 1, (ties, unstable)


@pytest.mark.parametrize("N,H,ratio,order,with_pitch", [(1200, 480, 10000.0 / 48000.0, 13, True), (1200, 480, 0.25, 12, True),
                                                        (2400, 480, 0.5, 12, False), (2048, 1024, 0.5, 16, False),
                                                        (200, 100, 1.5, 8, False)])
def test_synthetic_frames_against_the_oracle(vb, oracle, pkg, N, H, ratio, order, with_pitch):
    """600 frames from sample_offset 3 * 48000 + 12345, no frame left out: on these the oracle alone has status 0 everywhere and
    moves by less than 1e-6 under a 1e-13 perturbation, so every frame must meet the tolerance itself."""
    F = 600
    d = vb.synth_speech((F - 1) * H + N, sample_offset=OFFSET)
    sig = d.numpy()
    params = pkg.AnalysisParams.make(SR, lpc_order=0, formant_order=order, est_init=_est0(pkg), mfcc=None)
    ext = pkg.AnalysisExt.make(ratio, rms=True)
    rec, st = _ex(vb, d, params, ext, N, H, F)
    d.free()
    frames = [sig[t * H:t * H + N] for t in range(F)]
    ties, unstable = _check_against_oracle(oracle, rec, st, frames, oracle.window("hanning", N), (SR, 0.2, 75.0, 600.0), SR * ratio,
                                           ratio, order, _est0(pkg), with_pitch=with_pitch)
    print(f"{N}/{H} r {ratio:.4f} p {order}: pitch top ties {ties}, oracle-unstable frames {unstable}")
    assert unstable == 0 and ties <= 1, (ties, unstable)


# ---- 3. PCM -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("N,H,ratio,order", [(500, 100, 10000.0 / 44100.0, 13), (1200, 480, 10000.0 / 48000.0, 12),
                                             (1200, 480, 0.25, 12)])
def test_pcm_equals_widen_then_f64(vb, pkg, audio, N, H, ratio, order, tracked):
    F = 300
    n = (F - 1) * H + N
    s = np.clip(np.rint(audio[:n] * 20000.0), -32768, 32767).astype(np.int16)
    s[7 * H + 3] = -32768
    raw = vb.to_device(np.concatenate([np.zeros(1, np.int16), s]), np.int16)
    pcm_ptr = raw.ptr + 2                                      # the PCM base at 2 mod 4
    assert pcm_ptr % 4 == 2
    wide = vb.empty(n)
    vb.pcm16_to_f64(pcm_ptr, out=wide)
    params = _params(pkg, order)
    ext = pkg.AnalysisExt.make(ratio, rms=True)
    track = pkg.PitchTrackParams.make(kmax=4) if tracked else None
    got = _ex(vb, pcm_ptr, params, ext, N, H, F, track=track, pcm=True, lists=tracked)
    want = _ex(vb, wide, params, ext, N, H, F, track=track, lists=tracked)
    seq, seq_st, _, _ = _sequence(vb, pkg, wide, params, ext, N, H, F, track=track)
    raw.free(); wide.free()
    _assert_records(f"pcm {N}/{H}", got[0], got[1], want[0], want[1], params, ext)
    _assert_records(f"pcm {N}/{H} against the sequence", got[0], got[1], seq, seq_st, params, ext)
    for a, b in zip(got[3:], want[3:]):                        # count, peak, index (the lists' unlisted tail is nobody's)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 4. the degenerate forms -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H", [(1200, 480), (500, 100)])
def test_an_ext_that_asks_for_nothing_is_the_plain_call(vb, pkg, audio, N, H):
    F = 300
    x_d = vb.to_device(audio[:(F - 1) * H + N])
    seg = np.array([0, 50, 51], np.int64)
    params = _params(pkg, 12)
    rec0, st0 = vb.analyze_frames(x_d, params, seg_start=seg, frame_len=N, stride=H, n_frames=F)
    for ext in (None, pkg.AnalysisExt.make(), pkg.AnalysisExt.make(1.0), pkg.AnalysisExt.make(0.0, formant_sample_rate=SR)):
        rec, st = _ex(vb, x_d, params, ext, N, H, F, seg=seg)
        assert rec.shape[1] == 36 and np.array_equal(_i64(rec), _i64(rec0[:, :36])) and np.array_equal(st, st0)
    # rms alone: exactly one more column, nothing else moves
    rec, st = _ex(vb, x_d, params, pkg.AnalysisExt.make(rms=True), N, H, F, seg=seg)
    assert rec.shape[1] == 37 and np.array_equal(_i64(rec[:, :36]), _i64(rec0[:, :36])) and np.array_equal(st, st0)
    assert np.array_equal(_i64(rec[:, 36]), _i64(vb.rms(x_d, frame_len=N, stride=H, n_frames=F)))
    x_d.free()


def test_with_a_track_it_is_the_tracked_call(vb, pkg, audio):
    N, H, F, kmax = 1200, 480, 300, 4
    x_d = vb.to_device(audio[:(F - 1) * H + N])
    seg = np.array([0, 50, 51], np.int64)
    params = _params(pkg, 12)
    track = pkg.PitchTrackParams.make(kmax=kmax)
    t_rec, t_st, t_cand, t_count, t_peak, t_index = vb.analyze_frames_tracked(x_d, params, track, seg_start=seg, frame_len=N, stride=H,
                                                                              n_frames=F, lists=True)
    listed = np.arange(kmax)[None, :] < t_count[:, None]
    for ext in (None, pkg.AnalysisExt.make(), pkg.AnalysisExt.make(0.25, rms=True), pkg.AnalysisExt.make(rms=True)):
        rec, st, cand, count, peak, index = _ex(vb, x_d, params, ext, N, H, F, seg=seg, track=track, lists=True)
        assert np.array_equal(_i64(rec[:, 0:2]), _i64(t_rec[:, 0:2])) and np.array_equal(index, t_index)
        assert np.array_equal(count, t_count) and np.array_equal(_i64(peak), _i64(t_peak)) and np.array_equal(st[0], t_st[0])
        assert np.array_equal(_i64(cand[listed]), _i64(t_cand[listed]))
        plain, plain_st = _ex(vb, x_d, params, ext, N, H, F, seg=seg)
        assert np.array_equal(_i64(rec[:, 2:]), _i64(plain[:, 2:])) and np.array_equal(st, plain_st)
        if ext is None or not ext.rms:
            assert np.array_equal(_i64(rec), _i64(t_rec[:, :36])) and np.array_equal(st, t_st)
    # without the peaks (silence_threshold 0, no outputs) the RMS kernel runs alone
    quiet = pkg.PitchTrackParams.make(kmax=kmax, silence_threshold=0.0)
    ext = pkg.AnalysisExt.make(0.25, rms=True)
    rec, st = _ex(vb, x_d, params, ext, N, H, F, seg=seg, track=quiet)
    plain, plain_st = _ex(vb, x_d, params, ext, N, H, F, seg=seg)
    assert np.array_equal(_i64(rec[:, 2:]), _i64(plain[:, 2:])) and np.array_equal(st, plain_st)
    x_d.free()


# ---- 5. segments -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,ratio,order", [(500, 100, 10000.0 / 44100.0, 13), (1200, 480, 0.25, 12)])
def test_three_utterances_of_unequal_length(vb, pkg, audio, N, H, ratio, order):
    F = 450
    seg = np.array([0, 37, 200], np.int64)
    x_d = vb.to_device(audio[:(F - 1) * H + N])
    params = _params(pkg, order)
    ext = pkg.AnalysisExt.make(ratio, rms=True)
    got, st = _ex(vb, x_d, params, ext, N, H, F, seg=seg)
    want, want_st, _, _ = _sequence(vb, pkg, x_d, params, ext, N, H, F, seg=seg)
    _assert_records(f"segments {N}/{H}", got, st, want, want_st, params, ext)
    # the estimates restart at every utterance: its first rows are those of a call that begins there
    for s0, s1 in ((37, 200), (200, F)):
        part, _ = _ex(vb, x_d.ptr + s0 * H * 8, params, ext, N, H, s1 - s0)
        assert np.array_equal(_i64(part[:, 2:10]), _i64(got[s0:s1, 2:10])), s0
    x_d.free()


# ---- 6. standalone ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,ratio,order", [(500, 100, 10000.0 / 44100.0, 13), (1200, 480, 0.25, 12), (4096, 2048, 0.5, 12)])
def test_find_formants_with_a_ratio(vb, pkg, audio, N, H, ratio, order):
    F = 120
    seg = np.array([0, 30], np.int64)
    x_d = vb.to_device(audio[:(F - 1) * H + N])
    rate = SR * ratio
    got = vb.find_formants(x_d, rate, order, _est0(pkg), seg_start=seg, frame_len=N, stride=H, n_frames=F, resample_ratio=ratio)
    direct = vb.last_burg_direct_count()
    m = int(vb.L.vbx_resampled_len(N, ratio))
    rs = vb.empty((F, m))
    vb.resample_linear(x_d, ratio, frame_len=N, stride=H, n_frames=F, out=rs)
    want = vb.find_formants(rs, rate, order, _est0(pkg), seg_start=seg, frame_len=m, stride=m, n_frames=F)
    assert direct == vb.last_burg_direct_count()
    for name in ("formants", "res", "count", "coeffs", "status"):
        assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name
    assert np.all(want["status"] == 0) and np.all(want["count"] > 0)
    # ratio 1.0 is vbx_find_formants_f64 itself
    same = vb.find_formants(rs, rate, order, _est0(pkg), seg_start=seg, frame_len=m, stride=m, n_frames=F, resample_ratio=1.0)
    assert np.array_equal(same["formants"].view(np.uint8), want["formants"].view(np.uint8))
    rs.free(); x_d.free()


# ---- 7. layouts ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,ratio,order,pcm,tracked", [(1200, 481, 10000.0 / 48000.0, 12, False, False),
                                                         (1200, 481, 0.25, 12, False, True),
                                                         (1200, 481, 0.25, 12, True, False),
                                                         (500, 101, 10000.0 / 44100.0, 13, True, True),
                                                         (200, 101, 1.5, 8, False, False)])
def test_odd_bases_odd_stride_and_padded_records(vb, pkg, audio, N, H, ratio, order, pcm, tracked):
    """x at 8 mod 16 (PCM: 2 mod 16), an odd stride, records padded to an even ld, status3 at 4 mod 16: bit-equal to the aligned dense
    [F, N] call, fences and padding intact (the fences are NaN / -32768: a sample read outside a frame would show)."""
    F, kmax = 37, 4
    sig = audio[24000:24000 + (F - 1) * H + N]
    if pcm:
        sig = np.clip(np.rint(sig * 20000.0), -32768, 32767).astype(np.int16)
    params = _params(pkg, order)
    ext = pkg.AnalysisExt.make(ratio, rms=True)
    track = pkg.PitchTrackParams.make(kmax=kmax) if tracked else None
    width = _width(vb, params, ext)
    assert width == 37
    ld = width + 7
    seg = np.array([0, 9, 10], np.int64)
    dense_d = vb.to_device(la.windows(sig, N, H, F).reshape(-1))
    want = _ex(vb, dense_d, params, ext, N, N, F, seg=seg, track=track, pcm=pcm, lists=tracked)
    dense_d.free()
    a = la.Arena(la.DeviceBackend(vb), f"analyze_ex {N}/{H} pcm={pcm} tracked={tracked}")
    a.input("x", sig, residue=2 if pcm else 8)
    a.output("records", np.float64, F, width, ld=ld, residue=0)
    a.output("status3", np.int32, 3, F, residue=4)
    a.output("peak", np.float64, F, 1, residue=8)
    a.output("index", np.int32, F, 1, residue=8)
    a.place()
    outs = pkg.PitchTrackOutputs(None, None, a["peak"], a["index"])
    fn = vb.L.vbx_analyze_frames_ex_pcm16 if pcm else vb.L.vbx_analyze_frames_ex_f64

    def call(rec_ptr):
        return fn(vb.ctx, a["x"], F, N, H, C.byref(params), C.byref(ext), None if track is None else C.byref(track),
                  seg.ctypes.data, seg.size, rec_ptr, ld, a["status3"], C.byref(outs) if tracked else None)
    assert call(a["records"] + 8) == E_INVALID                 # records at 8 mod 16
    assert call(a["records"]) == 0, vb.L.vbx_last_error(vb.ctx)
    got = a.finish()
    la.assert_written(a.label, "records", got["records"])
    la.assert_same_bits(a.label, "records", got["records"], np.ascontiguousarray(want[0]))
    la.assert_same_bits(a.label, "status3", got["status3"], want[1])
    if tracked:
        la.assert_same_bits(a.label, "peak", got["peak"][:, 0], want[4])
        la.assert_same_bits(a.label, "index", got["index"][:, 0], want[5])


# ---- 8. misuse -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pcm", [False, True])
def test_rejected_calls_write_nothing_and_leave_the_context_usable(vb, pkg, audio, pcm):
    N, H, F = 1200, 480, 64
    sig = audio[:(F - 1) * H + N]
    if pcm:
        sig = np.clip(np.rint(sig * 20000.0), -32768, 32767).astype(np.int16)
    x = vb.to_device(sig)
    fn = vb.L.vbx_analyze_frames_ex_pcm16 if pcm else vb.L.vbx_analyze_frames_ex_f64
    params = _params(pkg, 12)
    good = pkg.AnalysisExt.make(0.25, rms=True)
    REC = _width(vb, params, good) + 1                         # 38
    canary = {"records": np.full((F, REC), la.CANARY_F64, np.uint64), "status3": np.full((3, F), la.CANARY_I32, np.uint32),
              "peak": np.full(F, la.CANARY_F64, np.uint64), "index": np.full(F, la.CANARY_I32, np.uint32)}
    dev = {k: vb.to_device(v) for k, v in canary.items()}
    outs = pkg.PitchTrackOutputs(None, None, dev["peak"].ptr, dev["index"].ptr)

    def call(x_ptr=x.ptr, n=F, n_len=N, hop=H, p=params, e=good, track=None, rec=dev["records"].ptr, ld=REC):
        return fn(vb.ctx, x_ptr, n, n_len, hop, None if p is None else C.byref(p), None if e is None else C.byref(e),
                  None if track is None else C.byref(track), None, 0, rec, ld, dev["status3"].ptr,
                  C.byref(outs) if track is not None else None)

    def variant(**kw):
        q = _params(pkg, 12)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    E = pkg.AnalysisExt.make
    bad = [dict(e=E(v)) for v in (-0.25, float("nan"), float("inf"), -float("inf"), 64.5, 1e9)]
    bad += [dict(e=E(0.25, formant_sample_rate=v)) for v in (-1.0, float("nan"), float("inf"))]
    bad += [dict(e=E(0.0, formant_sample_rate=float("nan"), rms=True))]
    bad += [dict(e=E(0.0005)),                                 # m = 1
            dict(e=E(1e-9)),                                   # m = 1
            dict(e=E(0.25), p=variant(formant_order=63)),      # an order Burg refuses
            dict(e=E(0.25, rms=True), p=variant(formant_order=0, n_est=0))]       # a ratio without formants
    # what the plain and the tracked call reject
    bad += [dict(p=None), dict(ld=REC - 2), dict(ld=REC - 1), dict(rec=dev["records"].ptr + 8), dict(rec=None), dict(x_ptr=None),
            dict(n_len=0), dict(hop=0), dict(n_len=(1 << 26) + 1), dict(n=1 << 31), dict(p=variant(n_est=7)),
            dict(p=variant(mfcc_coeffs=65)), dict(p=variant(lpc_order=1200)), dict(n_len=3, hop=1),
            dict(track=pkg.PitchTrackParams.make(kmax=0)), dict(track=pkg.PitchTrackParams.make(kmax=64)),
            dict(track=pkg.PitchTrackParams.make(kmax=4, octave_cost=float("nan")))]
    for b in bad:
        assert call(**b) == E_INVALID, b
        assert vb.L.vbx_last_error(vb.ctx)
    vb.sync()
    for k, d in dev.items():                                   # nothing was written
        assert np.array_equal(d.numpy().view(np.uint8), np.ascontiguousarray(canary[k]).view(np.uint8)), k
    assert call(n=0) == 0 and call(n=0, e=None) == 0           # an empty batch succeeds
    for k in ("records", "status3"):
        assert np.array_equal(dev[k].numpy().view(np.uint8), np.ascontiguousarray(canary[k]).view(np.uint8)), k
    assert call() == 0, vb.L.vbx_last_error(vb.ctx)            # ... and the next valid call is right
    rec = dev["records"].numpy().view(np.float64)[:, :REC - 1]
    want, want_st = _ex(vb, x, params, good, N, H, F, pcm=pcm)
    assert np.array_equal(_i64(rec), _i64(want)) and np.array_equal(dev["status3"].numpy().view(np.int32), want_st)
    assert np.all(dev["records"].numpy()[:, REC - 1] == la.CANARY_F64)      # the padding column is nobody's
    # the standalone entry point rejects the same ratios
    if not pcm:
        est = _est0(pkg)
        o = vb.empty((F, 4, 2))
        for r in (-0.25, float("nan"), 64.5, 0.0005):
            assert vb.L.vbx_find_formants_resampled_f64(vb.ctx, x.ptr, F, N, H, SR, r, 12, None, 0, est.ctypes.data, 4, o.ptr, None, None,
                                                        None, None) == E_INVALID, r
        o.free()
    for d in list(dev.values()) + [x]:
        d.free()


# ---- 9. one call, no dense batch ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pcm", [False, True])
@pytest.mark.parametrize("ratio,burg", [(10000.0 / 48000.0, "burg_resampled"), (0.25, "burg_lags_resampled")])
def test_no_dense_batch_and_nothing_widened(pkg, pcm, ratio, burg):
    N, H, F = 1200, 480, 400
    ctx = pkg.VoxBox(0)
    try:
        x = ctx.synth_speech((F - 1) * H + N, sample_offset=OFFSET)
        if pcm:
            s = np.clip(np.rint(x.numpy() * 20000.0), -32768, 32767).astype(np.int16)
            x.free()
            x = ctx.to_device(s, np.int16)
        params = _params(pkg, 12)
        ext = pkg.AnalysisExt.make(ratio, rms=True)
        fn = ctx.analyze_frames_ex_pcm16 if pcm else ctx.analyze_frames_ex
        reps = {}
        for name, track in (("plain", None), ("tracked", pkg.PitchTrackParams.make(kmax=4))):
            fn(x, params, ext, track, frame_len=N, stride=H, n_frames=F)             # tables, workspaces
            ctx.profile_reset(); ctx.profile(True)
            fn(x, params, ext, track, frame_len=N, stride=H, n_frames=F)
            reps[name] = (ctx.profile_report(), ctx.profile_streams())
            ctx.profile(False)
        x.free()
    finally:
        ctx.close()
    for name, (rep, streams) in reps.items():
        rms = "frame_rms_peak" if name == "tracked" else "frame_rms"
        for k in ("analyze", burg, rms):
            assert k in rep and rep[k][1] == 1, (name, k, sorted(rep))
        assert streams["analyze"] == 0 and streams[burg] == 1 and streams[rms] == 1, streams     # the chain and the RMS beside the spectral kernel
        for k in ("resample", "pcm16", "rms", "burg", "burg_lags", "frame_peak", "frame_peak_pcm16"):
            assert k not in rep, (name, k, sorted(rep))
