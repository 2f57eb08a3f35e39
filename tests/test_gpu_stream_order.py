"""The stream contract of include/voxbox_hip.h -- "calls are asynchronous on the context's HIP stream", "contexts are independent of
each other" -- on a CALLER-CREATED stream, with no host wait between the caller's producer, the call and the caller's consumer.
Every other GPU test uses the session context (a stream the library owns) and reads results through vbx_memcpy_d2h, which drains
that stream: a dropped hipStreamWaitEvent, an upload skipped while its first copy is in flight or a workspace overwritten by the
next call while the side stream still reads it would pass all of them.

  A  the late producer (tests/stream_harness.py late_producer): behind a delay of milliseconds, the input is copied into place ON
     the stream, the call follows, a device copy of every output follows the call; the host has run ahead (hipStreamQuery), and
     after one synchronisation the copies equal the call bracketed by vbx_sync, bit for bit.  One case per ordering mechanism of
     the vbx_api_*.hip units; which mechanism ran is asserted from the profile of the synchronised pass.  One case makes the side stream LATE
     (a sequential tracker scan several times longer than the fused kernel), so that a missing join shows.
  B  a fixed list of calls queued behind a delay with ONE synchronisation at the end, forward and reversed: neighbours share
     workspace slots at different sizes, alternate between two segment lists and two estimate sets (re-upload and skip-upload of the
     pinned staging buffers), and a stand-alone main-stream call reads what a fused call uploaded on the side stream.
  C  two contexts on two streams, interleaved; vbx_last_error stays per context; one is destroyed while the other has work queued.
  D  the torch recipe of INTEGRATION.md section 3 in a child process, on a torch.cuda.Stream and on torch's default stream.

Vacuity conditions are assertions: the delay's measured length, the not-ready query, the tracker-to-analyze ratio, the stream of
each kernel.  test_zz_report prints what was measured and writes it to the file VBX_STREAM_ORDER_REPORT names (profiles/stream_order/)."""
import ctypes as C
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import analyze_reference as ar
import parity_asserts as pa
import pitch_path_model as ppm
import stream_harness as sh
from conftest import rel_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
f64, f32, i32, i16 = np.float64, np.float32, np.int32, np.int16
REPORT = {"late_producer": {}, "queue": {}, "two_contexts": {}, "torch": {}}
SEG_A, SEG_B = np.array([0, 5], dtype=np.int64), np.array([0, 8], dtype=np.int64)       # same size, different content


# ---- fixtures ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hip(pkg, vb):
    return sh.Hip(pkg)


@pytest.fixture(scope="module")
def speech(vb):
    """22 s of the synthetic speech the other GPU tests use, from the same offset (8.4 MB: the sliced tracker's shape rule)."""
    d = vb.synth_speech(1_056_000, sample_offset=2 * 48000)
    a = d.numpy()
    d.free()
    return a


@pytest.fixture(scope="module")
def wav_speech(golden_dir):
    with wave.open(os.path.join(golden_dir, "sample-two_vowels.wav"), "rb") as w:
        sr = float(w.getframerate())
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return sr, pcm.astype(f64) / 32767.0


class Ctx:
    """A fresh context on a caller-created stream, with its Delay."""

    def __init__(self, pkg, hip, lpc_policy=None):
        self.pkg, self.hip = pkg, hip
        self.stream = hip.stream_create()
        self.vb = pkg.VoxBox(0, self.stream, lpc_policy)
        self.delay = sh.Delay(self.vb, pkg)

    def close(self):
        if self.vb is not None:
            self.vb.sync()
            self.vb.close()
            self.hip.stream_sync(self.stream)
            self.hip.stream_destroy(self.stream)
            self.vb = None


@pytest.fixture
def sctx(pkg, hip):
    made = []

    def make(lpc_policy=None):
        made.append(Ctx(pkg, hip, lpc_policy))
        return made[-1]
    yield make
    for c in made:
        c.close()


def est_set(pkg, which="male"):
    return np.array([[f, 1.0] for f in (pkg.MALE_FORMANT_ESTIMATES if which == "male" else pkg.FEMALE_FORMANT_ESTIMATES)])


def to_pcm(x):
    return np.round(x * (0.9 * 32767.0)).astype(i16)


def run_case(name, c, call, inputs, outputs, probe=None):
    r = sh.late_producer(c.vb, c.stream, call, inputs, outputs, c.delay, hip=c.hip, probe=probe)
    REPORT["late_producer"][name] = {k: r[k] for k in ("call_ms", "delay_ms", "delay_batches", "probe", "streams", "times")}
    return r


def on_stream(r, sid, *names):
    for n in names:
        assert r["streams"].get(n) == sid, f"{n}: expected stream {sid}, profile {r['streams']}"


def absent(r, *names):
    for n in names:
        assert n not in r["streams"], f"{n} ran: {r['streams']}"


def any_on_stream(r, sid, names):
    assert any(r["streams"].get(n) == sid for n in names), f"none of {names} on stream {sid}: {r['streams']}"


TRACKERS = ("tracker", "tracker_chunked")
BURGS = ("burg", "burg_lags", "burg_long", "burg_lags_resampled", "burg_resampled")
LPCS = ("autocorr_lpc", "autocorr_fewlags", "autocorr_fft", "autocorr_tiles", "autocorr_long", "levinson_rows", "lpc_rows")


# ---- A: the fused frame loop -------------------------------------------------------------------------------------------------

def analyze_setup(c, audio, N, H, F, sr, seg, mfcc, pcm=False, est="male"):
    """Buffers and parameters of one fused call on c: (x, host input, params, records, status3, ld)."""
    vb, pkg = c.vb, c.pkg
    n = (F - 1) * H + N
    host = to_pcm(audio[:n]) if pcm else np.ascontiguousarray(audio[:n])
    x = vb.empty(n, i16 if pcm else f64)
    prm = pkg.AnalysisParams.make(sr, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=12, est_init=est_set(pkg, est), mfcc=mfcc)
    rec_w = int(vb.L.vbx_record_doubles(C.byref(prm)))
    ld = rec_w + (rec_w & 1)
    return x, host, prm, vb.empty((F, ld)), vb.empty((3, F), i32), ld


@pytest.mark.parametrize("name,N,H,F,sr,seg", [
    ("fused_1200_seg_a", 1200, 480, 300, SR, [0, 100]), ("fused_1200_seg_b", 1200, 480, 300, SR, [0, 37, 211]),
    ("unfused_256", 256, 128, 300, 16000.0, [0, 100]), ("long_5000", 5000, 2500, 9, SR, [0, 4])])
def test_analyze_frames_f64_late_producer(pkg, oracle, speech, sctx, name, N, H, F, sr, seg):
    c = sctx()
    seg = np.array(seg, dtype=np.int64)
    mfcc = (13, 100.0, 8000.0) if sr == SR else (13, 100.0, 7000.0)
    x, host, prm, rec, st3, ld = analyze_setup(c, speech, N, H, F, sr, seg, mfcc)

    def call():
        c.vb.analyze_frames(x, prm, seg_start=seg, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=ld, status=st3)
    r = run_case("analyze_f64/" + name, c, call, [(x, host)], [rec, st3])
    if N == 1200:
        on_stream(r, 0, "analyze", "lpc_rows")
        on_stream(r, 1, "formant_resonances")
        any_on_stream(r, 1, TRACKERS)
        any_on_stream(r, 1, BURGS)
        absent(r, "pitch", "mfcc")
    elif N == 256:                                           # no fused kernel: LPC and MFCC beside the formant chain, pitch alone
        on_stream(r, 0, "pitch")
        on_stream(r, 1, "formant_resonances", "mfcc")
        any_on_stream(r, 1, LPCS)
        any_on_stream(r, 1, TRACKERS)
        absent(r, "analyze")
    else:                                                    # "side" is the context's own stream
        assert r["streams"] and all(s == 0 for s in r["streams"].values()), r["streams"]
        on_stream(r, 0, "pitch_long", "burg_long", "mfcc_long", "formant_resonances")
    if name == "fused_1200_seg_a":                           # equal to the synchronised call is equal to RIGHT: the oracle
        grec, gst = r["ref"]
        sub = 160
        orec, ost, _, _ = ar.oracle_records(oracle, speech, N, H, range(sub), SR, (0.2, 75.0, 600.0), 12, 12, est_set(pkg), mfcc, set(seg.tolist()))
        assert np.array_equal(gst[:, :sub], ost)
        assert np.all((orec[:, 0] == 0.0) == (grec[:sub, 0] == 0.0)), "voiced / unvoiced decision differs"
        assert np.all(np.abs(grec[:sub, 0] - orec[:, 0]) <= 1e-4 * np.abs(orec[:, 0])) and np.all(np.abs(grec[:sub, 1] - orec[:, 1]) <= 1e-4)
        assert np.all(np.abs(grec[:sub, 2:10:2] - orec[:, 2:10:2]) <= 1e-4 * np.abs(orec[:, 2:10:2]))
        for t in range(sub):
            assert np.all(rel_close(grec[t, 10:23], orec[t, 10:23])) and np.all(rel_close(grec[t, 23:36], orec[t, 23:36])), t


@pytest.mark.parametrize("N,H,widened", [(1200, 480, False), (1024, 512, True)])
def test_analyze_frames_pcm16_late_producer(pkg, speech, sctx, N, H, widened):
    c = sctx()
    F, seg = 300, np.array([0, 100], dtype=np.int64)
    x, host, prm, rec, st3, ld = analyze_setup(c, speech, N, H, F, SR, seg, (13, 100.0, 8000.0), pcm=True)

    def call():
        c.vb.analyze_frames_pcm16(x, prm, seg_start=seg, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=ld, status=st3)
    r = run_case(f"analyze_pcm16/{N}", c, call, [(x, host)], [rec, st3])
    on_stream(r, 0, "analyze")
    on_stream(r, 1, "formant_resonances")
    if widened:
        on_stream(r, 0, "pcm16")                             # the widening pass, on the main stream ahead of the fork
    else:
        absent(r, "pcm16")                                   # the kernels read the PCM directly
    # the records are those of the widened samples through the f64 call (the header's promise), which the case above holds to the oracle
    wide = (host.astype(f64) / 32767.0)
    xd = c.vb.to_device(wide)
    ref64, _ = c.vb.analyze_frames(xd, prm, seg_start=seg, frame_len=N, stride=H, n_frames=F, record_ld=ld)
    xd.free()
    assert sh.bits_equal(ref64, r["ref"][0])


def track_params(pkg):
    """kmax 4 and a silence threshold at which the frame peaks decide the unvoiced score of the quiet (unvoiced) frames."""
    return pkg.PitchTrackParams.make(kmax=4, silence_threshold=0.2)


@pytest.mark.parametrize("N,H,sr", [(1200, 480, SR), (256, 128, 16000.0)])
@pytest.mark.parametrize("lists", ["owned", "supplied"])
def test_analyze_frames_tracked_late_producer(pkg, speech, sctx, N, H, sr, lists):
    c = sctx()
    F, seg = 400, np.array([0, 150], dtype=np.int64)
    mfcc = (13, 100.0, 8000.0) if sr == SR else (13, 100.0, 7000.0)
    off = 48000 if N == 1200 else 71000                      # both windows straddle the recording's unvoiced second
    x, host, prm, rec, st3, ld = analyze_setup(c, speech[off:], N, H, F, sr, seg, mfcc)
    trk = track_params(pkg)
    outs, bufs = None, []
    if lists == "supplied":
        bufs = [c.vb.empty((F, 4, 2)), c.vb.empty(F, i32), c.vb.empty(F), c.vb.empty(F, i32)]
        outs = tuple(bufs)

    def call():
        c.vb.analyze_frames_tracked(x, prm, trk, seg_start=seg, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=ld, status=st3,
                                    outputs=outs)
    r = run_case(f"tracked_f64/{N}/{lists}", c, call, [(x, host)], [rec, st3] + bufs)
    on_stream(r, 0, "pitch_path_spec", "pitch_path_write")
    on_stream(r, 1, "frame_peak", "formant_resonances")      # the peaks are taken on the side stream: the path waits for ev_peak
    if N == 1200:
        on_stream(r, 0, "analyze")
    else:
        on_stream(r, 0, "pitch")
        # queued on the side stream AHEAD of the peak kernel (analyze_frames_impl; the profile has no order, only streams).  Both
        # finish long before the pitch kernel on stream 0 does (0.02 + 0.006 ms against 0.2 ms, profiles/stream_order/): a missing
        # ev_peak wait cannot show here or at any other shape of this call, and no test of this file claims to catch it
        on_stream(r, 1, "mfcc")
    grec = r["ref"][0]
    assert np.any(grec[:, 0] > 0) and np.any(grec[:, 0] == 0), "the contour should have voiced and unvoiced frames"
    if lists == "supplied":                                  # the path over the call's own lists is the model's, bit for bit
        cand, cnt, peak, idx = r["ref"][2:]
        par = dict(trk.path.as_dict(), time_step=H / sr)
        mp, mi = ppm.pitch_path(cand, cnt, r["ref"][1][0], peak, seg, par)
        assert sh.bits_equal(np.ascontiguousarray(grec[:, 0:2]), mp) and np.array_equal(idx, mi)


@pytest.mark.parametrize("form,tracked", [("f64", True), ("pcm16", False)])
def test_analyze_frames_ex_late_producer(pkg, oracle, speech, sctx, form, tracked):
    """The frame loop of examples/formant_extraction: 500 / 100 at 44.1 kHz, formants at ratio 10000 / 44100 and order 13, RMS column."""
    c = sctx()
    N, H, F, sr = 500, 100, 300, 44100.0
    seg = np.array([0, 100], dtype=np.int64)
    n = (F - 1) * H + N
    pcm = form == "pcm16"
    host = to_pcm(speech[:n]) if pcm else np.ascontiguousarray(speech[:n])
    x = c.vb.empty(n, i16 if pcm else f64)
    prm = pkg.AnalysisParams.make(sr, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=13, est_init=est_set(pkg), mfcc=(13, 100.0, 8000.0))
    ext = pkg.AnalysisExt.make(10000.0 / 44100.0, 0.0, rms=True)
    w = int(c.vb.L.vbx_record_doubles_ex(C.byref(prm), C.byref(ext)))
    ld = w + (w & 1)
    rec, st3 = c.vb.empty((F, ld)), c.vb.empty((3, F), i32)
    trk = track_params(pkg) if tracked else None
    fn = c.vb.analyze_frames_ex_pcm16 if pcm else c.vb.analyze_frames_ex

    def call():
        fn(x, prm, ext, trk, seg_start=seg, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=ld, status=st3)
    r = run_case(f"analyze_ex/{form}", c, call, [(x, host)], [rec, st3])
    on_stream(r, 1, "frame_rms_peak" if tracked else "frame_rms", "formant_resonances")
    any_on_stream(r, 1, ("burg_lags_resampled", "burg_resampled"))
    any_on_stream(r, 0, ("analyze", "pitch"))
    # the RMS column is RMS::rms of the rectangular frame, the formant columns find_formants at the ratio (the oracle's restatement)
    grec, gst = r["ref"]
    samples = host.astype(f64) / 32767.0 if pcm else host
    est = est_set(pkg)
    for t in range(120):
        fr = samples[t * H:t * H + N]
        assert rel_close(grec[t, w - 1], oracle.rms(fr)).all(), t
        if t in (0, 100):
            est = est_set(pkg)
        got = oracle.find_formants_ratio(fr, 10000.0, 10000.0 / 44100.0, 13, est)
        s, est = got[0], got[1]
        assert s == gst[1, t]
        assert np.all(np.abs(grec[t, 2:10:2] - est[:, 0]) <= 1e-4 * np.abs(est[:, 0])), (t, grec[t, 2:10], est)


# ---- A: the formant chain ----------------------------------------------------------------------------------------------------

def test_find_formants_late_producer(pkg, oracle, speech, sctx):
    c = sctx()
    N, H, F = 512, 160, 300
    seg, est0 = np.array([0, 100], dtype=np.int64), est_set(pkg)
    n = (F - 1) * H + N
    host = np.ascontiguousarray(speech[:n])
    x = c.vb.empty(n)
    bufs = {"formants": c.vb.empty((F, 4, 2)), "res": c.vb.empty((F, 32, 2)), "count": c.vb.empty(F, i32), "coeffs": c.vb.empty((F, 12)),
            "status": c.vb.empty(F, i32)}

    def call():
        c.vb.find_formants(x, SR, 12, est0, seg_start=seg, frame_len=N, stride=H, n_frames=F, out=bufs)
    r = run_case("find_formants/512", c, call, [(x, host)], list(bufs.values()))
    on_stream(r, 0, "formant_resonances")
    any_on_stream(r, 0, TRACKERS)
    any_on_stream(r, 0, BURGS)
    ff, st = r["ref"][0], r["ref"][4]
    est = est0.copy()
    for t in range(F):
        if t in (0, 100):
            est = est0.copy()
        s, est, _, _ = oracle.find_formants(host[t * H:t * H + N], SR, 12, est)
        assert s == st[t]
        assert np.all(np.abs(est[:, 0] - ff[t, :, 0]) <= 1e-4 * np.abs(est[:, 0])), (t, est, ff[t])


def test_find_formants_time_sliced_late_producer(pkg, speech, sctx, monkeypatch):
    """64 equal utterances of 1024 frames at stride 16 (65,536 frames, 8 MB of audio: the shape rule tests/test_gpu_regressions.py
    documents) under VBX_TRACKER_CHUNKED=0: Burg and the root finder of slice j + 1 on the context's stream beside the tracker of
    slice j on its own, joined by ev_trk."""
    monkeypatch.setenv("VBX_TRACKER_CHUNKED", "0")
    c = sctx()
    N, H, seg_len, n_seg = 512, 16, 1024, 64
    F = seg_len * n_seg
    seg, est0 = np.arange(0, F, seg_len, dtype=np.int64), est_set(pkg)
    n = (F - 1) * H + N
    host = np.ascontiguousarray(speech[:n])
    x = c.vb.empty(n)
    bufs = {"formants": c.vb.empty((F, 4, 2)), "status": c.vb.empty(F, i32)}

    def call():
        c.vb.find_formants(x, SR, 12, est0, seg_start=seg, frame_len=N, stride=H, n_frames=F, out=bufs)
    r = run_case("find_formants/time_sliced", c, call, [(x, host)], list(bufs.values()))
    on_stream(r, 2, "tracker")
    on_stream(r, 0, "formant_resonances")
    absent(r, "tracker_chunked")
    # right: the chunked scan of the same batch (the default dispatch, held to the oracle elsewhere) gives the same rows
    monkeypatch.setenv("VBX_TRACKER_CHUNKED", "1")
    xd = c.vb.to_device(host)
    ref = c.vb.find_formants(xd, SR, 12, est0, seg_start=seg, frame_len=N, stride=H, n_frames=F, want=("formants", "status"))
    xd.free()
    assert sh.bits_equal(ref["formants"], r["ref"][0]) and np.array_equal(ref["status"], r["ref"][1])


def test_fused_call_with_a_late_side_stream(pkg, speech, sctx, monkeypatch):
    """One utterance of 3000 frames under VBX_TRACKER_CHUNKED=0: the formant tracker is the sequential one-lane scan, far longer
    than the fused kernel on the context's stream, so the side stream finishes LAST and only the join keeps the consumer behind it."""
    monkeypatch.setenv("VBX_TRACKER_CHUNKED", "0")
    c = sctx()
    N, H, F = 1200, 16, 3000
    x, host, prm, rec, st3, ld = analyze_setup(c, speech, N, H, F, SR, None, (13, 100.0, 8000.0))

    def call():
        c.vb.analyze_frames(x, prm, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=ld, status=st3)
    r = run_case("analyze_f64/late_side_stream", c, call, [(x, host)], [rec, st3])
    on_stream(r, 0, "analyze")
    on_stream(r, 1, "tracker")
    ratio = r["times"]["tracker"] / max(r["times"]["analyze"], 1e-6)
    REPORT["late_producer"]["analyze_f64/late_side_stream"]["tracker_to_analyze"] = round(ratio, 2)
    assert ratio >= 5.0, f"vacuous: tracker {r['times']['tracker']} ms on the side stream, analyze {r['times']['analyze']} ms"
    assert np.all(np.isfinite(r["ref"][0][:, 2:10]))         # the formant columns: written for every frame, and the reference's


# ---- A: the stand-alone entry points -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("whole", [False, True])
def test_pitch_split_form_late_producer(pkg, oracle, speech, sctx, whole):
    """4096 / 2048: the refinement in kernels of its own with the lag curves in WS_CURVE (kmax 1), and the whole list."""
    c = sctx()
    N, H, F = 4096, 2048, 120
    kmax = pkg.pitch_max_candidates(N) if whole else 1
    n = (F - 1) * H + N
    host = np.ascontiguousarray(speech[:n])
    x, win = c.vb.empty(n), c.vb.window(pkg.WINDOW_HANNING, N)
    outs = (c.vb.empty((F, kmax, 2)), c.vb.empty(F, i32), c.vb.empty(F, i32))

    def call():
        c.vb.pitch(x, SR, 0.2, 75.0, 600.0, kmax=kmax, frame_len=N, stride=H, n_frames=F, window=win, out=outs)

    def probe(v):
        return {"split": int(v.L.vbx_internal_last_spectral_split(v.ctx)), "form": int(v.L.vbx_internal_last_pitch_form(v.ctx))}
    r = run_case(f"pitch/4096/{'whole' if whole else 'kmax1'}", c, call, [(x, host)], list(outs), probe)
    on_stream(r, 0, "pitch")
    assert r["probe"]["form"] // 100 >= 3                    # an FFT kernel
    if whole:
        assert r["probe"]["form"] % 100 in (1, 2), r["probe"]
    else:
        assert r["probe"]["form"] % 100 == 0 and r["probe"]["split"] == 1, r["probe"]
    cand, cnt, st = r["ref"]
    w = oracle.window("hanning", N)
    for t in range(0, F, 5):
        s, ec, en = oracle.pitch(host[t * H:t * H + N] * w, SR, 0.2, 75.0, 600.0, cap=2)
        assert s == st[t] and (s != 0 or en == cnt[t]), (t, s, st[t], en, cnt[t])
        if s != 0:
            continue
        assert ar.classify_top(cand[t, 0], ec, en) in ("ok", "swap"), (t, cand[t, 0], ec)


def test_pitch_path_late_producer(pkg, speech, sctx):
    """vbx_pitch_path_f64 with segments: lists, counts, statuses and peaks all arrive late."""
    c = sctx()
    N, H, F, K = 1200, 480, 1500, 4
    seg = np.array([0, 400, 401, 1100], dtype=np.int64)
    xd = c.vb.to_device(speech[:(F - 1) * H + N])
    cand_h, cnt_h, st_h = c.vb.pitch(xd, SR, 0.2, 75.0, 600.0, kmax=K, frame_len=N, stride=H, n_frames=F, window=c.vb.window(pkg.WINDOW_HANNING, N))
    peak_h = c.vb.frame_peak(xd, frame_len=N, stride=H, n_frames=F)
    xd.free()
    par = pkg.PitchPathParams.make(time_step=H / SR, silence_threshold=0.2)
    cand, cnt, st, peak = c.vb.empty((F, K, 2)), c.vb.empty(F, i32), c.vb.empty(F, i32), c.vb.empty(F)
    outs = (c.vb.empty((F, 2)), c.vb.empty(F, i32))

    def call():
        c.vb.pitch_path(cand, cnt, st, peak, seg_start=seg, params=par, n_frames=F, kmax=K, out=outs)
    r = run_case("pitch_path/segments", c, call, [(cand, cand_h), (cnt, cnt_h), (st, st_h), (peak, peak_h)], list(outs))
    on_stream(r, 0, "pitch_path_peak", "pitch_path_spec", "pitch_path_write")
    mp, mi = ppm.pitch_path(cand_h, cnt_h, st_h, peak_h, seg, par.as_dict())
    assert sh.bits_equal(r["ref"][0], mp) and np.array_equal(r["ref"][1], mi)


def test_autocorr_lpc_exact_policy_late_producer(pkg, oracle, wav_speech, sctx):
    """Frames of the golden recording the conditioning probe hands to the double-double recursion (k_lpc_exact.hip)."""
    c = sctx(pkg.LPC_POLICY_EXACT)
    wsr, audio = wav_speech
    N, H, P = 1024, 256, 12
    F = min(400, pkg.frame_count(audio.size, N, H))
    n = (F - 1) * H + N
    host = np.ascontiguousarray(audio[:n])
    x, win = c.vb.empty(n), c.vb.window(pkg.WINDOW_HANNING, N)
    outs = (c.vb.empty((F, P + 1)), c.vb.empty((F, P + 1)))

    def call():
        c.vb.autocorr_lpc(x, P, frame_len=N, stride=H, n_frames=F, window=win, out=outs)
    r = run_case("autocorr_lpc/exact", c, call, [(x, host)], list(outs), lambda v: v.last_lpc_exact_count())
    assert r["probe"] > 0, "no row of this material was listed for the exact recursion"
    on_stream(r, 0, "lpc_exact_list")
    # the lag sums against the oracle (the LPC rows of listed frames are held to the exact row by tests/test_gpu_lpc_exact.py)
    w = oracle.window("hanning", N)
    xw = np.stack([host[t * H:t * H + N] * w for t in range(0, F, 7)])
    pa.autocorr_lpc_rows(oracle, xw, P, False, r["ref"][0][::7], None, "exact", lpc=False)


def test_lpc_burg_direct_rows_late_producer(pkg, oracle, speech, sctx):
    """The one-pass Burg at 1024 / order 12 on the synthetic speech with a silent frame among it: its guard hands the silent
    frame and about one frame in a hundred of the speech to the direct recursion (a device-side list, WS_BURG_LIST)."""
    c = sctx()
    N, P, F = 1024, 12, 300
    fr = np.ascontiguousarray(speech[:F * N].reshape(F, N)).copy()
    fr[65] = 0.0                                             # (a silent frame: Err(LPC) in the reference, handed on by the guard)
    x = c.vb.empty((F, N))
    outs = (c.vb.empty((F, P)), c.vb.empty(F, i32))

    def call():
        c.vb.lpc_praat(x, P, frame_len=N, stride=N, n_frames=F, out=outs)
    r = run_case("lpc_burg/direct_rows", c, call, [(x, fr)], list(outs), lambda v: v.last_burg_direct_count())
    assert r["probe"] > 0, r["probe"]
    on_stream(r, 0, "burg_lags", "burg_direct_list")
    rows = sorted(set(range(0, F, 3)) | {65})
    pa.burg_rows(oracle, fr[rows], P, r["ref"][0][rows], r["ref"][1][rows], "burg")


@pytest.mark.parametrize("N,hi,form", [(1103, 16000.0, 3), (5000, 8000.0, 7)])
def test_mfcc_late_producer(pkg, oracle, speech, sctx, N, hi, form):
    """1103 samples with the upper band edge at 16 kHz: the chirp-z kernel (WS_CZT); 5000: the long-frame kernel."""
    c = sctx()
    H, F = (441, 300) if N == 1103 else (2500, 40)
    n = (F - 1) * H + N
    host = np.ascontiguousarray(speech[:n])
    x, win = c.vb.empty(n), c.vb.window(pkg.WINDOW_HANNING, N)
    outs = (c.vb.empty((F, 13)), c.vb.empty(F, i32))

    def call():
        c.vb.mfcc(x, 13, (100.0, hi), SR, frame_len=N, stride=H, n_frames=F, window=win, out=outs)
    r = run_case(f"mfcc/{N}", c, call, [(x, host)], list(outs), lambda v: int(v.L.vbx_internal_last_mfcc_form(v.ctx)))
    assert r["probe"] == form, r["probe"]
    on_stream(r, 0, "mfcc_long" if form == 7 else "mfcc")
    w = oracle.window("hanning", N)
    step = 6 if N == 1103 else 4
    xw = np.stack([host[t * H:t * H + N] * w for t in range(0, F, step)])
    pa.mfcc_rows(oracle, xw, 13, 100.0, hi, SR, r["ref"][0][::step], r["ref"][1][::step], f"mfcc {N}")


def test_f32_entry_points_late_producer(pkg, oracle, speech, sctx):
    """vbx_pitch_f32_wide (widened into WS_F32_IN, narrowed from WS_F32_OUT) and vbx_autocorr_lpc_f32 on float frames."""
    c = sctx()
    vb, N, F, P = c.vb, 1024, 200, 12
    fr = np.ascontiguousarray(speech[:F * N].reshape(F, N)).astype(f32)
    x = vb.empty((F, N), f32)
    cand, cnt, st = vb.empty((F, 4, 2), f32), vb.empty(F, i32), vb.empty(F, i32)

    def call_pitch():
        vb._check(vb.L.vbx_pitch_f32_wide(vb.ctx, x.ptr, F, N, N, None, SR, 0.2, 75.0, 600.0, 4, cand.ptr, cnt.ptr, st.ptr))
    r = run_case("pitch_f32_wide/1024", c, call_pitch, [(x, fr)], [cand, cnt, st])
    on_stream(r, 0, "widen_frames", "pitch", "narrow")
    xd = vb.to_device(fr.astype(f64))
    c64, n64, s64 = vb.pitch(xd, SR, 0.2, 75.0, 600.0, kmax=4, frame_len=N, stride=N, n_frames=F)     # as tests/test_gpu_f32.py holds it
    xd.free()
    pa.rounded_once(r["ref"][0], c64, "pitch_f32_wide")
    assert np.array_equal(r["ref"][1], n64) and np.array_equal(r["ref"][2], s64)
    rr, aa = vb.empty((F, P + 1), f32), vb.empty((F, P + 1), f32)

    def call_lpc():
        vb._check(vb.L.vbx_autocorr_lpc_f32(vb.ctx, x.ptr, F, N, N, None, P, 0, rr.ptr, aa.ptr))
    r = run_case("autocorr_lpc_f32/1024", c, call_lpc, [(x, fr)], [rr, aa])
    assert r["streams"] and all(s == 0 for s in r["streams"].values()), r["streams"]
    pa.autocorrelate_f32_rows(oracle, fr[::9], P + 1, r["ref"][0][::9], "autocorr_lpc_f32")
    pa.lpc_f32_rows(oracle, r["ref"][0][::9], P, r["ref"][1][::9], what="autocorr_lpc_f32")


# ---- B: a queue with no host waits in one context -------------------------------------------------------------------------------

def build_queue(c, pkg, speech, wav_speech):
    """[(name, call, outputs)]: about a dozen calls whose neighbours share workspace slots at different sizes (WS_COEFFS / WS_RES /
    WS_COUNT / WS_STATUS / WS_TRK / WS_BURG_LIST / WS_ROOTS_LIST: every formant chain; WS_MISC / WS_UNSURE: the spectral kernels;
    WS_F32_IN / WS_F32_OUT: the PCM widening and the f32 form; WS_LONG / WS_LONG2: 5000-sample frames; WS_CZT; WS_CURVE: 4096
    split; WS_LPC_LIST; WS_PATH / WS_PATH_TAB; WS_TRACK: context-owned lists; WS_EX: the dense resample fallback; WS_SEG / WS_EST:
    every call with segments), that alternate SEG_A / SEG_B and the male / female estimates with one repeated pair, and in which a
    stand-alone main-stream call reads WS_SEG / WS_EST a fused call uploaded on the side stream."""
    vb = c.vb
    steps = []
    han = {n: vb.window(pkg.WINDOW_HANNING, n) for n in (1024, 1103, 4096)}

    def analyze(name, N, H, F, seg, est, pcm=False, sr=SR, tracked=False, ext=None, off=0):
        x, host, prm, rec, st3, ld = analyze_setup(c, speech[off:], N, H, F, sr, seg, (13, 100.0, 8000.0 if sr == SR else 7000.0), pcm=pcm, est=est)
        vb._check(vb.L.vbx_memcpy_h2d(vb.ctx, x.ptr, host.ctypes.data, host.nbytes))
        trk = track_params(pkg) if tracked else None
        if ext is not None:
            w = int(vb.L.vbx_record_doubles_ex(C.byref(prm), C.byref(ext)))
            ld = w + (w & 1)
            rec = vb.empty((F, ld))
        kw = dict(seg_start=seg, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=ld, status=st3)
        if ext is not None:
            call = lambda: vb.analyze_frames_ex(x, prm, ext, trk, **kw)
        elif tracked:
            call = lambda: vb.analyze_frames_tracked(x, prm, trk, **kw)
        elif pcm:
            call = lambda: vb.analyze_frames_pcm16(x, prm, **kw)
        else:
            call = lambda: vb.analyze_frames(x, prm, **kw)
        steps.append((name, call, [rec, st3]))

    def formants(name, N, H, F, seg, est):
        x = vb.to_device(speech[7000:7000 + (F - 1) * H + N])
        bufs = {"formants": vb.empty((F, 4, 2)), "res": vb.empty((F, 32, 2)), "count": vb.empty(F, i32), "status": vb.empty(F, i32)}
        e = est_set(pkg, est)
        steps.append((name, lambda: vb.find_formants(x, SR, 12, e, seg_start=seg, frame_len=N, stride=H, n_frames=F, out=bufs), list(bufs.values())))
        return bufs

    # the resonance rows a stand-alone tracker call reads: computed once, before the queue
    rows = formants("rows", 512, 160, 300, SEG_A, "male")
    steps.pop()[1]()
    vb.sync()

    def estimate(name, seg, est):
        out, e = vb.empty((300, 4, 2)), est_set(pkg, est)
        steps.append((name, lambda: vb._check(vb.L.vbx_estimate_formants_f64(
            vb.ctx, rows["res"].ptr, 300, 32, seg.ctypes.data, seg.size, e.ctypes.data, 4, rows["status"].ptr, out.ptr)), [out]))

    analyze("analyze 1200 A male", 1200, 480, 300, SEG_A, "male")                       # uploads A / male on the SIDE stream
    estimate("estimate_formants A male", SEG_A, "male")                                # main stream, same content: no upload
    analyze("tracked 256 B female", 256, 128, 500, SEG_B, "female", sr=16000.0, tracked=True)   # re-upload of both; WS_TRACK, WS_PATH
    formants("find_formants 512 B female", 512, 160, 200, SEG_B, "female")              # the repeated pair: skipped
    analyze("pcm16 1024 A male", 1024, 512, 150, SEG_A, "male", pcm=True)               # WS_F32_IN: the widened copy
    fr32 = np.ascontiguousarray(speech[:100 * 512].reshape(100, 512)).astype(f32)
    x32, c32, n32, s32 = vb.to_device(fr32, f32), vb.empty((100, 2, 2), f32), vb.empty(100, i32), vb.empty(100, i32)
    steps.append(("pitch_f32_wide 512", lambda: vb._check(vb.L.vbx_pitch_f32_wide(
        vb.ctx, x32.ptr, 100, 512, 512, None, SR, 0.2, 75.0, 600.0, 2, c32.ptr, n32.ptr, s32.ptr)), [c32, n32, s32]))   # WS_F32_IN / _OUT, smaller
    analyze("analyze 5000 B male", 5000, 2500, 9, SEG_B, "male")                        # WS_LONG / WS_LONG2; side == the context's stream
    xm, om, sm = vb.to_device(speech[:299 * 441 + 1103]), vb.empty((300, 13)), vb.empty(300, i32)
    steps.append(("mfcc 1103 czt", lambda: vb.mfcc(xm, 13, (100.0, 16000.0), SR, frame_len=1103, stride=441, n_frames=300,
                                                  window=han[1103], out=(om, sm)), [om, sm]))
    xp, op = vb.to_device(speech[:39 * 2048 + 4096]), (vb.empty((40, 1, 2)), vb.empty(40, i32), vb.empty(40, i32))
    steps.append(("pitch 4096 split", lambda: vb.pitch(xp, SR, 0.2, 75.0, 600.0, kmax=1, frame_len=4096, stride=2048, n_frames=40,
                                                      window=han[4096], out=op), list(op)))
    wsr, wav = wav_speech
    Fw = min(200, pkg.frame_count(wav.size, 1024, 256))
    xw, ow = vb.to_device(wav[:(Fw - 1) * 256 + 1024]), (vb.empty((Fw, 13)), vb.empty((Fw, 13)))
    steps.append(("autocorr_lpc exact", lambda: vb.autocorr_lpc(xw, 12, frame_len=1024, stride=256, n_frames=Fw, window=han[1024], out=ow), list(ow)))
    # the pitch path twice over the same lists with the two segment lists: its chunk table (staging buffer 2) re-uploaded
    Fp = 700
    xq = vb.to_device(speech[:(Fp - 1) * 480 + 1200])
    lists = (vb.empty((Fp, 4, 2)), vb.empty(Fp, i32), vb.empty(Fp, i32))
    vb.pitch(xq, SR, 0.2, 75.0, 600.0, kmax=4, frame_len=1200, stride=480, n_frames=Fp, window=vb.window(pkg.WINDOW_HANNING, 1200), out=lists)
    pk = vb.empty(Fp)
    vb.frame_peak(xq, frame_len=1200, stride=480, n_frames=Fp, out=pk)
    vb.sync()
    par = pkg.PitchPathParams.make(time_step=0.01, silence_threshold=0.05)
    for nm, sg in (("pitch_path A", SEG_A), ("pitch_path B", SEG_B)):
        o = (vb.empty((Fp, 2)), vb.empty(Fp, i32))
        steps.append((nm, (lambda sg=sg, o=o: vb.pitch_path(lists[0], lists[1], lists[2], pk, seg_start=sg, params=par, n_frames=Fp, kmax=4, out=o)), list(o)))
    analyze("ex tracked 4096 A female (dense resample)", 4096, 2048, 30, SEG_A, "female", tracked=True,
            ext=pkg.AnalysisExt.make(0.5, 0.0, rms=True))                                  # m = 2048 > 1280: WS_EX
    frb = np.ascontiguousarray(speech[:120 * 1024].reshape(120, 1024)).copy()
    frb[5] = 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(1024) / SR)
    xb, ob = vb.to_device(frb), (vb.empty((120, 12)), vb.empty(120, i32))
    steps.append(("lpc_burg 1024", lambda: vb.lpc_praat(xb, 12, frame_len=1024, stride=1024, n_frames=120, out=ob), list(ob)))   # WS_BURG_LIST
    analyze("analyze 1200 A male again, 123 frames", 1200, 480, 123, SEG_A, "male", off=48000)
    return steps


# kernels of the queue's synchronised pass, by the workspace their launcher owns: formant chain (WS_COEFFS / RES / COUNT / STATUS,
# WS_TRK, WS_BURG_LIST, WS_ROOTS_LIST), spectral kernels (WS_MISC / WS_UNSURE), pcm16 + widen / narrow (WS_F32_IN / _OUT), the long-frame
# kernels (WS_LONG / WS_LONG2), lpc_exact_list (WS_LPC_LIST), the path (WS_PATH / WS_PATH_TAB), frame_peak into context-owned lists
# (WS_TRACK), resample (WS_EX: the dense fallback); the chirp-z MFCC (WS_CZT) and the split pitch (WS_CURVE) share the names mfcc / pitch
# with other forms: part A asserts those forms from the library's probes at the same shapes
QUEUE_KERNELS = ("analyze", "pitch", "tracker", "formant_resonances", "burg_lags", "burg_direct_list", "burg_long", "pcm16", "widen_frames",
                 "narrow", "pitch_long", "mfcc_long", "mfcc", "lpc_exact_list", "pitch_path_spec", "pitch_path_write", "frame_peak",
                 "frame_rms_peak", "resample", "autocorr_lpc")
# calls from the front of each order before any staged array changes for the second time inside the queue
QUEUE_PREFIX = {"forward": 4, "reversed": 2}


def test_queue_without_host_waits(pkg, speech, wav_speech, sctx):
    c = sctx()
    vb = c.vb
    steps = build_queue(c, pkg, speech, wav_speech)
    assert 12 <= len(steps) <= 16
    for _, call, _ in steps:                                 # warm-up: tables, workspaces at their largest sizes
        call()
    vb.sync()
    for _, _, outs in steps:                                 # (bytes no call writes -- row padding -- read the same in every pass)
        for o in outs:
            vb._check(vb.L.vbx_memset(vb.ctx, o.ptr, 0xFF, o.nbytes))
    vb.sync()
    ref = []
    vb.profile(True)
    vb.profile_reset()
    vb.timer_begin()
    for _, call, outs in steps:                              # the pass that synchronises after every call
        call()
        vb.sync()
        ref.append([o.numpy() for o in outs])
    total_ms = vb.timer_end()
    ran = vb.profile_streams()
    vb.profile(False)
    # the kernels whose launchers own the slots the docstring of build_queue names (a dispatch change that drops one shows here)
    for name in QUEUE_KERNELS:
        assert name in ran, f"{name} did not run in the queue: {sorted(ran)}"
    reps = c.delay.reps_for(total_ms / sh.DELAY_FACTOR)      # the whole list is "the call": a delay >= 10 ms and >= the list itself
    delay_ms = c.delay.timed(reps)
    assert delay_ms >= sh.DELAY_MIN_MS and delay_ms >= total_ms, f"vacuous: the delay took {delay_ms} ms, the list {total_ms} ms"
    REPORT["queue"] = {"calls": [s[0] for s in steps], "synchronised_pass_ms": round(total_ms, 3), "delay_ms": round(delay_ms, 3),
                       "kernels": sorted(ran)}
    for order, idx in (("forward", list(range(len(steps)))), ("reversed", list(reversed(range(len(steps)))))):
        for _, _, outs in steps:
            for o in outs:
                vb._check(vb.L.vbx_memset(vb.ctx, o.ptr, 0xFF, o.nbytes))
        vb.sync()
        c.delay.queue(reps)
        early = None
        for n_done, i in enumerate(idx):
            steps[i][1]()
            if n_done + 1 == QUEUE_PREFIX[order]:
                early = c.hip.stream_query(c.stream)
        state = c.hip.stream_query(c.stream)
        c.hip.stream_sync(c.stream)
        vb.sync()
        # Up to here no staged array has changed TWICE inside the queue (the first change finds its previous upload long done):
        # nothing the header lists as blocking has happened, so the host must be ahead of the delay.  Further on a second change
        # waits for the first one's upload (test_host_blocks_only_as_documented), which is behind the delay: by the end the host
        # has been held back, and whether it is still ahead is recorded, not asserted.
        assert early == sh.HIP_ERROR_NOT_READY, f"{order}: the host was not ahead after {QUEUE_PREFIX[order]} calls ({early})"
        REPORT["queue"][order + "_host_ahead_at_the_end"] = state == sh.HIP_ERROR_NOT_READY
        for i in idx:
            for k, o in enumerate(steps[i][2]):
                got = o.numpy()
                assert sh.bits_equal(got, ref[i][k]), (order, steps[i][0], k, sh.first_difference(got, ref[i][k]))


SEG_X, SEG_Y = np.array([0, 200, 300], dtype=np.int64), np.array([0, 100, 300], dtype=np.int64)   # same size; frames 200-299 are the unvoiced second


def staged_calls(c, pkg, speech):
    """Two entry points whose results depend on the three staged host arrays, on c: find_formants (segment starts, initial
    estimates) and the pitch path (its chunk table), each as call(seg, est, out); plus an allocator of their outputs."""
    vb, N, H, F, K = c.vb, 1200, 480, 700, 4
    x = vb.to_device(speech[:(F - 1) * H + N])
    lists = (vb.empty((F, K, 2)), vb.empty(F, i32), vb.empty(F, i32))
    vb.pitch(x, SR, 0.2, 75.0, 600.0, kmax=K, frame_len=N, stride=H, n_frames=F, window=vb.window(pkg.WINDOW_HANNING, N), out=lists)
    pk = vb.empty(F)
    vb.frame_peak(x, frame_len=N, stride=H, n_frames=F, out=pk)
    vb.sync()
    par = pkg.PitchPathParams.make(time_step=H / SR, silence_threshold=0.2)

    def outputs():
        return [vb.empty((F, 4, 2)), vb.empty(F, i32), vb.empty((F, 2)), vb.empty(F, i32)]

    def call(seg, est, o):
        vb.find_formants(x, SR, 12, est, seg_start=seg, frame_len=N, stride=H, n_frames=F, out={"formants": o[0], "status": o[1]})
        vb.pitch_path(lists[0], lists[1], lists[2], pk, seg_start=seg, params=par, n_frames=F, kmax=K, out=(o[2], o[3]))
    return outputs, call


def test_staged_arrays_follow_their_content(pkg, speech, sctx):
    """The skip-if-unchanged upload of the segment starts, the initial estimates and the path's chunk table: a call must compute
    with ITS arrays, whatever an earlier call of the same context staged at the same size.  The reference of each content comes
    from a fresh context whose FIRST upload it is (an upload that cannot be skipped), so it does not share the staging state of
    the context under test; the two contents must give different results, or the comparison would prove nothing."""
    contents = {"x": (SEG_X, est_set(pkg, "male")), "y": (SEG_Y, est_set(pkg, "female"))}
    ref = {}
    for k, (seg, est) in contents.items():
        f = sctx()
        outputs, call = staged_calls(f, pkg, speech)
        o = outputs()
        call(seg, est, o)
        f.vb.sync()
        ref[k] = [b.numpy() for b in o]
    assert not sh.bits_equal(ref["x"][0], ref["y"][0]), "vacuous: the formant tracks do not depend on the segment list / estimates"
    assert not sh.bits_equal(ref["x"][2], ref["y"][2]), "vacuous: the pitch path does not depend on the segment list"
    c = sctx()
    outputs, call = staged_calls(c, pkg, speech)
    order = ["x", "y", "y", "x", "y"]
    outs = [outputs() for _ in order]
    call(*contents["x"], outs[0])                             # warm: tables, workspaces, and content x staged
    c.vb.sync()
    for o in outs:
        for b in o:
            c.vb._check(c.vb.L.vbx_memset(c.vb.ctx, b.ptr, 0xFF, b.nbytes))
    c.vb.sync()
    c.delay.queue(c.delay.reps_for(2.0))
    for k, o in zip(order, outs):
        call(*contents[k], o)
    c.hip.stream_sync(c.stream)
    c.vb.sync()
    for n, (k, o) in enumerate(zip(order, outs)):
        for j, b in enumerate(o):
            got = b.numpy()
            assert sh.bits_equal(got, ref[k][j]), (n, k, j, sh.first_difference(got, ref[k][j]))


def test_host_blocks_only_as_documented(pkg, speech, sctx):
    """The conventions of include/voxbox_hip.h: a warm call does not block the host -- not with unchanged host arrays, and not
    with changed ones whose previous upload has long run; a call that changes an array AGAIN while the previous change's upload
    is still queued waits for that upload, i.e. for the work queued ahead of it.  Host wall time of each call behind a delay of
    >= 40 ms: the first three return within a quarter of it with the stream not ready, the fourth only after half of it."""
    import time
    c = sctx()
    outputs, call = staged_calls(c, pkg, speech)
    x_, y_ = (SEG_X, est_set(pkg, "male")), (SEG_Y, est_set(pkg, "female"))
    o = [outputs() for _ in range(4)]
    call(*y_, o[0])
    call(*x_, o[0])                                          # warm at both contents; x is what is staged now
    c.vb.sync()
    reps = c.delay.reps_for(40.0 / sh.DELAY_FACTOR)          # 1.5 x 40 ms
    delay_ms = c.delay.timed(reps)
    assert delay_ms >= 40.0, f"vacuous: the delay took {delay_ms} ms"
    c.delay.queue(reps)
    t, states = [], []
    for content, out in ((x_, o[0]), (x_, o[1]), (y_, o[2]), (x_, o[3])):   # unchanged, unchanged, first change, second change
        t0 = time.perf_counter()
        call(*content, out)
        t.append(1e3 * (time.perf_counter() - t0))
        states.append(c.hip.stream_query(c.stream))
    c.hip.stream_sync(c.stream)
    c.vb.sync()
    REPORT["queue"]["host_ms_per_call_unchanged_unchanged_changed_changed_again"] = [round(v, 3) for v in t]
    REPORT["queue"]["blocking_delay_ms"] = round(delay_ms, 3)
    assert all(v <= 0.25 * delay_ms for v in t[:3]) and states[:3] == [sh.HIP_ERROR_NOT_READY] * 3, (t, states, delay_ms)
    assert t[3] >= 0.5 * delay_ms - sum(t[:3]), (t, delay_ms)


# ---- C: two contexts ---------------------------------------------------------------------------------------------------------

def test_two_contexts_interleaved(pkg, speech, sctx):
    a, b = sctx(), sctx()

    def calls_of(c, shapes):
        out = []
        for N, H, F, seg, est, tracked, sr in shapes:
            x, host, prm, rec, st3, ld = analyze_setup(c, speech, N, H, F, sr, seg, (13, 100.0, 8000.0 if sr == SR else 7000.0), est=est)
            c.vb._check(c.vb.L.vbx_memcpy_h2d(c.vb.ctx, x.ptr, host.ctypes.data, host.nbytes))
            kw = dict(seg_start=seg, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=ld, status=st3)
            if tracked:
                trk = track_params(pkg)
                out.append((lambda c=c, x=x, prm=prm, trk=trk, kw=kw: c.vb.analyze_frames_tracked(x, prm, trk, **kw), [rec, st3]))
            else:
                out.append((lambda c=c, x=x, prm=prm, kw=kw: c.vb.analyze_frames(x, prm, **kw), [rec, st3]))
        return out
    ca = calls_of(a, [(1200, 480, 300, SEG_A, "male", False, SR), (512, 256, 411, SEG_B, "female", True, SR), (1200, 480, 77, SEG_B, "male", False, SR)])
    cb = calls_of(b, [(256, 128, 500, SEG_B, "female", True, 16000.0), (1103, 441, 200, SEG_A, "male", False, SR), (1024, 512, 333, SEG_A, "female", False, SR)])

    def solo(c, calls):
        for call, _ in calls:
            call()
        c.vb.sync()
        for _, outs in calls:
            for o in outs:
                c.vb._check(c.vb.L.vbx_memset(c.vb.ctx, o.ptr, 0xFF, o.nbytes))
        c.vb.sync()
        ref = []
        c.vb.timer_begin()
        for call, outs in calls:
            call()
            c.vb.sync()
            ref.append([o.numpy() for o in outs])
        return ref, c.vb.timer_end()
    (ref_a, ms_a), (ref_b, ms_b) = solo(a, ca), solo(b, cb)
    # one deliberately invalid call on A (n_lags = 0: refused before anything is launched), as tests/test_gpu_api_errors.py does
    la, lb = a.vb.L, b.vb.L
    scratch = a.vb.zeros(4096)
    msg_b0 = lb.vbx_last_error(b.vb.ctx)
    assert la.vbx_autocorrelate_f64(a.vb.ctx, scratch.ptr, 4, 512, 512, None, 0, scratch.ptr) == -1
    msg_a, msg_b = la.vbx_last_error(a.vb.ctx), lb.vbx_last_error(b.vb.ctx)
    assert b"n_lags" in msg_a and msg_b == msg_b0 and b"n_lags" not in msg_b

    def poison(c, calls):
        for _, outs in calls:
            for o in outs:
                c.vb._check(c.vb.L.vbx_memset(c.vb.ctx, o.ptr, 0xFF, o.nbytes))
        c.vb.sync()

    def check(calls, ref, what):
        for i, (_, outs) in enumerate(calls):
            for k, o in enumerate(outs):
                got = o.numpy()
                assert sh.bits_equal(got, ref[i][k]), (what, i, k, sh.first_difference(got, ref[i][k]))
    ra, rb = a.delay.reps_for(ms_a / sh.DELAY_FACTOR), b.delay.reps_for(ms_b / sh.DELAY_FACTOR)
    # interleaved, no host waits; each context's message stays its own
    poison(a, ca), poison(b, cb)
    a.delay.queue(ra), b.delay.queue(rb)
    for (call_a, _), (call_b, _) in zip(ca, cb):
        call_a()
        assert la.vbx_last_error(a.vb.ctx) == msg_a and lb.vbx_last_error(b.vb.ctx) == msg_b
        call_b()
        assert la.vbx_last_error(a.vb.ctx) == msg_a and lb.vbx_last_error(b.vb.ctx) == msg_b
    ahead = (a.hip.stream_query(a.stream), b.hip.stream_query(b.stream))
    a.hip.stream_sync(a.stream), b.hip.stream_sync(b.stream)
    a.vb.sync(), b.vb.sync()
    assert ahead == (sh.HIP_ERROR_NOT_READY, sh.HIP_ERROR_NOT_READY), f"the host did not run ahead of both streams: {ahead}"
    check(ca, ref_a, "A interleaved"), check(cb, ref_b, "B interleaved")
    # B is destroyed while A still has work queued (A's delay is made the longer one): A's results are unchanged
    poison(a, ca), poison(b, cb)
    delay_b = b.delay.timed(rb)
    ra_long = a.delay.reps_for(max(ms_a, 4.0 * (delay_b + ms_b)) / sh.DELAY_FACTOR)
    a.delay.queue(ra_long), b.delay.queue(rb)
    for (call_a, _), (call_b, _) in zip(ca, cb):
        call_b()
        call_a()
    state_a = a.hip.stream_query(a.stream)                   # (asked BEFORE: freeing B's memory makes the runtime wait for the device)
    b.close()
    a.hip.stream_sync(a.stream)
    a.vb.sync()
    assert state_a == sh.HIP_ERROR_NOT_READY, "vacuous: A had nothing queued any more when B was destroyed"
    check(ca, ref_a, "A after B was destroyed")
    scratch.free()
    REPORT["two_contexts"] = {"solo_ms": [round(ms_a, 3), round(ms_b, 3)], "delay_batches": [ra, rb, ra_long]}


# ---- D: the torch recipe, in a child process -----------------------------------------------------------------------------------

def test_torch_recipe_in_a_child_process():
    """INTEGRATION.md section 3 with torch's producer and consumer around the call, on a torch.cuda.Stream and on torch's default
    stream (tests/torch_stream_child.py; torch stays out of this process)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_stream_child.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    REPORT["torch"] = res
    assert res["stream"]["equal"] and res["stream"]["host_ahead"], res
    assert res["default_stream"]["handle"] == 0, res          # what the recipe used to pass on: NULL, "own stream"
    assert res["default_stream"]["refused"] and "torch.cuda.Stream" in res["default_stream"]["message"], res
    # the path from_torch closes is still open to a caller who passes the handle on by hand: the child runs it once and the report
    # keeps whether its records equalled the synchronised call's (they need not differ on every run: it is a race, not asserted)
    assert res["handle_0_passed_by_hand"]["context_handle"] == 0, res


def test_zz_report():
    """Writes what the tests above measured: it reads this module's REPORT, so it runs last (its name) and only means something
    after them -- selected alone it fails with "no case ran"."""
    rep = json.dumps(REPORT, indent=1, sort_keys=True, default=str)
    print(rep)
    out = os.environ.get("VBX_STREAM_ORDER_REPORT")
    if out:
        with open(out, "w") as f:
            f.write(rep + "\n")
    assert REPORT["late_producer"], "no case ran"
