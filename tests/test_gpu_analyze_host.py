"""vbx_analyze_host on a real MI355X: the frame loop on a recording in HOST memory, chunk by chunk, against the resident call on the
same channel -- vbx_analyze_frames_ex_pcm16 for PCM16, _f32in for float32, _f64 on the converted samples for 24- / 32-bit PCM and
double.  Every output is compared BIT FOR BIT (uint64 views), as in tests/test_gpu_analyze_f32in.py: the records, the three status
rows and, tracked, the candidate lists, counts, peaks and path indices.  The context's vbx_internal_last_* probes are not compared:
after a host call they describe its last chunk only.  F = 650 frames: at chunk_frames 64 eleven chunks, at 200 a ragged last chunk
of 50, at 650 and 1000 one chunk.  Segments [0, 150, 200, 390, 600]: a start on a cut (200, 600), and one 10 frames before the cut
at 400, whose warm-up is those 10 frames."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import layout_arena as la
import stream_harness as sh

pytestmark = pytest.mark.gpu

SR = 48000.0
F = 650
NATIVE, WIDENED = (1200, 480), (1024, 512)
SEG5 = [0, 150, 200, 390, 600]
E_INVALID = -1
FORMATS = ["pcm16", "pcm16_stereo1", "pcm24", "pcm32_3ch2", "f32", "f32_stereo0", "f64"]
FORMS = ["plain", "tracked", "ext", "tracked_ext"]


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _params(pkg, **kw):
    kw.setdefault("est_init", np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES]))
    return pkg.AnalysisParams.make(SR, **kw)


def _form(pkg, form):
    """(ext, track) of a form: ext = find_formants at ratio 0.25 plus the RMS column; track = kmax 4 with the default costs, whose
    silence_threshold is 0.03: the frame peaks and the segment maximum matter"""
    ext = pkg.AnalysisExt.make(0.25, rms=True) if "ext" in form else None
    track = pkg.PitchTrackParams.make(kmax=4) if "tracked" in form else None
    assert track is None or track.path.silence_threshold > 0.0
    return ext, track


@pytest.fixture(scope="module")
def base(vb, golden_dir):
    """the recording as doubles in (-1, 1): the synthetic speech with a stretch of the golden 16-bit WAV in its middle"""
    n = (F - 1) * 512 + 1200
    d = vb.synth_speech(n, sample_offset=5 * 48000 + 321)
    x = d.numpy()
    d.free()
    with wave.open(os.path.join(golden_dir, "sample-two_vowels.wav"), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    m = min(pcm.size, 60_000)
    x[120_000:120_000 + m] = pcm[:m].astype(np.float64) / 32767.0
    return x


def _pack24(s):
    return np.ascontiguousarray(np.ascontiguousarray(s, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)


_REC = {}


def _recording(base, fmt, N, H):
    """(host audio as analyze_host takes it, keyword arguments, the selected channel for the resident call, which resident call)"""
    if (fmt, N, H) not in _REC:
        _REC[(fmt, N, H)] = _make_recording(base, fmt, N, H)
    return _REC[(fmt, N, H)]


def _make_recording(base, fmt, N, H):
    x = base[:(F - 1) * H + N] * 0.9
    other = np.roll(x, 777)[::-1].copy()                       # what the other channels hold: nothing like the one analysed
    if fmt.startswith("pcm16"):
        s, o = np.round(x * 32767.0).astype(np.int16), np.round(other * 32767.0).astype(np.int16)
        audio = s if fmt == "pcm16" else np.ascontiguousarray(np.stack([o, s], axis=1))
        return audio, dict(channel=0 if fmt == "pcm16" else 1), s, "pcm16"
    if fmt == "pcm24":
        s = np.round(x * 8388607.0).astype(np.int32)
        return _pack24(s), dict(format=2, channels=1), s.astype(np.float64) / np.float64(8388607.0), "f64"
    if fmt == "pcm32_3ch2":
        s, o = np.round(x * 2147483647.0).astype(np.int64).astype(np.int32), np.round(other * 2147483647.0).astype(np.int64).astype(np.int32)
        return np.ascontiguousarray(np.stack([o, o[::-1], s], axis=1)), dict(channel=2), s.astype(np.float64) / np.float64(2147483647.0), "f64"
    if fmt.startswith("f32"):
        s, o = x.astype(np.float32), other.astype(np.float32)
        audio = s if fmt == "f32" else np.ascontiguousarray(np.stack([s, o], axis=1))
        return audio, dict(channel=0), s, "f32in"
    return x.copy(), dict(channel=0), x.copy(), "f64"


_REF = {}


def _resident(vb, pkg, base, fmt, shape, form, seg, policy="EXACT"):
    """the resident call's outputs on the selected channel, computed once per (format, shape, form, segments, policy)"""
    key = (fmt, shape, form, None if seg is None else tuple(seg), policy)
    if key not in _REF:
        N, H = shape
        _, _, chan, which = _recording(base, fmt, N, H)
        ext, track = _form(pkg, form)
        fn = {"pcm16": vb.analyze_frames_ex_pcm16, "f32in": vb.analyze_frames_ex_f32in, "f64": vb.analyze_frames_ex}[which]
        got = fn(chan, _params(pkg), ext, track, seg_start=seg, frame_len=N, stride=H, n_frames=F, lists=track is not None)
        _REF[key] = got
    return _REF[key]


def _host(vb, pkg, base, fmt, shape, form, seg, chunk, audio=None):
    N, H = shape
    a, kw, _, _ = _recording(base, fmt, N, H)
    ext, track = _form(pkg, form)
    return vb.analyze_host(a if audio is None else audio, _params(pkg), ext, track, chunk_frames=chunk, seg_start=seg, frame_len=N, stride=H,
                           lists=track is not None, **kw)


def _assert_same(label, got, want, width):
    rec, st = got[0][:, :width], got[1]
    wrec, wst = want[0][:, :width], want[1]
    assert rec.shape == wrec.shape == (F, width), (label, rec.shape, wrec.shape)
    a, b = _u64(rec), _u64(wrec)
    assert np.array_equal(a, b), (label, "records: first differing (frame, column)", tuple(np.argwhere(a != b)[0]), int((a != b).sum()))
    assert np.array_equal(st, wst), (label, "status3", np.argwhere(st != wst)[:8])
    assert len(got) == len(want)
    if len(got) > 2:
        cand, count, peak, index = got[2:]
        wcand, wcount, wpeak, windex = want[2:]
        assert np.array_equal(count, wcount), (label, "count", np.argwhere(count != wcount)[:8])
        assert np.array_equal(index, windex), (label, "index", np.argwhere(index != windex)[:8])
        assert np.array_equal(_u64(peak), _u64(wpeak)), (label, "peak", np.argwhere(_u64(peak) != _u64(wpeak))[:8])
        keep = np.arange(cand.shape[1])[None, :] < count[:, None]             # (entries past a frame's count are not written)
        assert np.array_equal(_u64(cand)[keep], _u64(wcand)[keep]), (label, "candidate lists")


def _width(vb, pkg, form):
    ext, _ = _form(pkg, form)
    p = _params(pkg)
    return int(vb.L.vbx_record_doubles_ex(C.byref(p), None if ext is None else C.byref(ext)))


def _check(vb, pkg, base, fmt, shape, form, seg, chunk, policy="EXACT"):
    want = _resident(vb, pkg, base, fmt, shape, form, seg, policy)
    got = _host(vb, pkg, base, fmt, shape, form, seg, chunk)
    _assert_same(f"{fmt} {shape} {form} seg {seg} chunk {chunk} {policy}", got, want, _width(vb, pkg, form))
    return got


@pytest.fixture
def policy(vb, pkg):
    old = vb.lpc_policy

    def set_policy(name):
        vb.lpc_policy = getattr(pkg, "LPC_POLICY_" + name)
    yield set_policy
    vb.lpc_policy = old


# ---- 1. every format, both shapes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [NATIVE, WIDENED], ids=["1200/480", "1024/512"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format(vb, pkg, base, fmt, shape):
    _check(vb, pkg, base, fmt, shape, "tracked_ext", SEG5, 200)
    _check(vb, pkg, base, fmt, shape, "plain", None, 64)


# ---- 2. every cut, form and segment list ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seg", [None, SEG5], ids=["one utterance", "five utterances"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fmt", ["pcm16", "f64"])
def test_every_cut_at_the_native_shape(vb, pkg, base, fmt, form, seg):
    for chunk in (64, 200, 650, 1000):
        _check(vb, pkg, base, fmt, NATIVE, form, seg, chunk)


@pytest.mark.parametrize("seg", [None, SEG5], ids=["one utterance", "five utterances"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fmt", ["pcm16", "f32", "pcm24"])
def test_every_cut_at_the_widened_shape(vb, pkg, base, fmt, form, seg):
    for chunk in (64, 200, 650, 1000):
        _check(vb, pkg, base, fmt, WIDENED, form, seg, chunk)


def test_one_utterance_per_frame(vb, pkg, base):
    _check(vb, pkg, base, "pcm16", NATIVE, "tracked_ext", list(range(F)), 200)


@pytest.mark.parametrize("pol", ["EXACT", "REFERENCE"])
def test_lpc_policies(vb, pkg, base, policy, pol):
    policy(pol)
    for fmt in ("pcm16", "f32", "pcm24"):
        for form, seg in (("tracked_ext", SEG5), ("plain", None)):
            _check(vb, pkg, base, fmt, NATIVE, form, seg, 200, pol)


# ---- 3. what runs --------------------------------------------------------------------------------------------------------------------

def test_native_stays_native(vb, pkg, base):
    """Mono PCM16 and float32 at 1200 / 480: the chunks are read as they were uploaded -- no widening pass, no unpack launch."""
    for fmt in ("pcm16", "f32"):
        vb.profile(True)
        vb.profile_reset()
        try:
            _host(vb, pkg, base, fmt, NATIVE, "tracked_ext", SEG5, 200)
            rep = vb.profile_report()
        finally:
            vb.profile(False)
        assert "host_rows" in rep and rep["host_rows"][1] == 4, sorted(rep)
        for name in rep:
            assert name not in ("pcm16", "f32_to_f64") and not name.startswith("unpack_"), (fmt, name, sorted(rep))


def test_every_new_launch_is_profiled(vb, pkg, base):
    seen, streams = {}, {}
    for fmt in FORMATS:
        vb.profile(True)
        vb.profile_reset()
        try:
            _host(vb, pkg, base, fmt, NATIVE, "plain", None, 200)
            seen[fmt], streams[fmt] = vb.profile_report(), vb.profile_streams()
        finally:
            vb.profile(False)
    for fmt, name in (("pcm16_stereo1", "unpack_pcm16"), ("pcm24", "unpack_pcm24"), ("pcm32_3ch2", "unpack_pcm32"), ("f32_stereo0", "unpack_f32")):
        # four chunks: one unpack launch, one stitch and one copy of the rows each (the first chunk has nothing to stitch to)
        assert seen[fmt].get(name, (0, 0))[1] == 4 and seen[fmt]["host_rows"][1] == 4 and seen[fmt]["tracker_stitch"][1] == 3, (fmt, sorted(seen[fmt]))
        assert streams[fmt][name] == 0 and streams[fmt]["host_rows"] == 0 and streams[fmt]["tracker_stitch"] == 0, streams[fmt]
    assert not any(n.startswith("unpack_") for n in seen["f64"]) and seen["f64"]["host_rows"][1] == 4


# ---- 4. host memory and ordering -----------------------------------------------------------------------------------------------------

def test_pinned_and_pageable_memory_give_the_same_bits(vb, pkg, base):
    for fmt in ("pcm16", "pcm24"):
        a, _, _, _ = _recording(base, fmt, *NATIVE)
        pinned = vb.malloc_host(a.shape, a.dtype)
        pinned[...] = a
        want = _resident(vb, pkg, base, fmt, NATIVE, "tracked_ext", SEG5)
        got = _host(vb, pkg, base, fmt, NATIVE, "tracked_ext", SEG5, 200, audio=pinned)
        _assert_same(f"{fmt} pinned", got, want, _width(vb, pkg, "tracked_ext"))
        _assert_same(f"{fmt} pageable", _host(vb, pkg, base, fmt, NATIVE, "tracked_ext", SEG5, 200), want, _width(vb, pkg, "tracked_ext"))
        vb.free_host(pinned)


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_the_audio_may_be_overwritten_when_the_call_returns(vb, pkg, base, pinned):
    """Late consumer, producer reuse: the call returns when the last byte of h_audio has been read, kernels may still be running;
    the caller overwrites the recording at once and reads the records afterwards."""
    form, width = "tracked_ext", _width(vb, pkg, "tracked_ext")
    a, kw, _, _ = _recording(base, "pcm16_stereo1", *NATIVE)
    want = _resident(vb, pkg, base, "pcm16_stereo1", NATIVE, form, SEG5)
    buf = vb.malloc_host(a.shape, a.dtype) if pinned else np.empty_like(a)
    buf[...] = a
    ext, track = _form(pkg, form)
    ld = width + (width & 1)
    rec, st = vb.empty((F, ld)), vb.empty((3, F), np.int32)
    lists = [vb.empty((F, 4, 2)), vb.empty(F, np.int32), vb.empty(F), vb.empty(F, np.int32)]
    vb.sync()
    assert vb.analyze_host(buf, _params(pkg), ext, track, chunk_frames=64, seg_start=SEG5, frame_len=NATIVE[0], stride=NATIVE[1],
                           out=rec, record_ld=ld, status=st, outputs=tuple(lists), **kw) is None
    buf[...] = -12345                                          # no wait in between
    got = (rec.numpy(), st.numpy()) + tuple(d.numpy() for d in lists)
    _assert_same("audio overwritten on return", got, want, width)
    for d in [rec, st] + lists:
        d.free()
    if pinned:
        vb.free_host(buf)


def test_two_calls_back_to_back_without_a_wait(vb, pkg, base):
    """The staging slots, the copy stream and their events belong to the context and outlive a call, and a call returns while its
    kernels may still be queued: the NEXT call's first uploads must wait for the slots' last readers.  A delay keeps the stream busy,
    then two host calls follow with no wait between them -- two chunks each, so that neither waits for the device on its own account
    before its uploads are issued, and one utterance, so that no segment list's upload blocks the host either -- once through the unpack kernel (the two channels of one stereo buffer) and once on the path
    that reads the slots directly (two mono recordings).  Both calls' outputs are the resident calls', bit for bit."""
    form, width = "tracked_ext", _width(vb, pkg, "tracked_ext")
    N, H = NATIVE
    stereo, _, s1, _ = _recording(base, "pcm16_stereo1", N, H)
    s0 = np.ascontiguousarray(stereo[:, 0])
    ext, track = _form(pkg, form)
    ld = width + (width & 1)
    want = [vb.analyze_frames_ex_pcm16(ch, _params(pkg), ext, track, seg_start=None, frame_len=N, stride=H, n_frames=F, lists=True) for ch in (s0, s1)]
    # (a first call sizes the workspaces, which drains the streams: done here, outside the queue)
    vb.analyze_host(stereo, _params(pkg), ext, track, chunk_frames=400, seg_start=None, frame_len=N, stride=H, lists=True)
    delay = sh.Delay(vb, pkg)
    reps = delay.reps_for(1.0)
    for label, audios, kws in (("unpack", (stereo, stereo), (dict(channel=0), dict(channel=1))),
                               ("native mono", (s0, s1), (dict(channel=0), dict(channel=0)))):
        pinned = []
        for a in audios:
            pinned.append(vb.malloc_host(a.shape, a.dtype))
            pinned[-1][...] = a
        outs = [[vb.empty((F, ld)), vb.empty((3, F), np.int32), vb.empty((F, 4, 2)), vb.empty(F, np.int32), vb.empty(F), vb.empty(F, np.int32)]
                for _ in range(2)]
        vb.sync()
        assert delay.timed(reps) >= sh.DELAY_MIN_MS                  # (else the test is vacuous)
        delay.queue(reps)
        for buf, kw, o in zip(pinned, kws, outs):
            assert vb.analyze_host(buf, _params(pkg), ext, track, chunk_frames=400, seg_start=None, frame_len=N, stride=H, out=o[0],
                                   record_ld=ld, status=o[1], outputs=tuple(o[2:]), **kw) is None
        vb.sync()
        for i, o in enumerate(outs):
            _assert_same(f"{label}, call {i} of two queued back to back", tuple(d.numpy() for d in o), want[i], width)
        for d in sum(outs, []):
            d.free()
        for b in pinned:
            vb.free_host(b)


def test_sync_leaves_nothing_running(pkg, base):
    """A context on a caller-created stream: after vbx_sync that stream is idle (hipStreamQuery) -- the pinned recording and every
    output can be freed -- and every new launch ran on the context's stream.  (The copy stream is not queried: it is idle when the
    call returns by construction, since the call waits for its last upload, so that vbx_sync drains it too is not what this shows.)"""
    hip = sh.Hip(pkg)
    stream = hip.stream_create()
    c = pkg.VoxBox(0, stream)
    try:
        form, width = "tracked_ext", None
        a, kw, chan, _ = _recording(base, "pcm24", *NATIVE)
        ext, track = _form(pkg, form)
        p = _params(pkg)
        width = int(c.L.vbx_record_doubles_ex(C.byref(p), C.byref(ext)))
        ld = width + (width & 1)
        want = c.analyze_frames_ex(chan, p, ext, track, seg_start=SEG5, frame_len=NATIVE[0], stride=NATIVE[1], n_frames=F, lists=True)
        pinned = c.malloc_host(a.shape, a.dtype)
        pinned[...] = a
        rec, st = c.empty((F, ld)), c.empty((3, F), np.int32)
        lists = [c.empty((F, 4, 2)), c.empty(F, np.int32), c.empty(F), c.empty(F, np.int32)]
        c.profile(True)
        c.profile_reset()
        c.analyze_host(pinned, p, ext, track, chunk_frames=200, seg_start=SEG5, frame_len=NATIVE[0], stride=NATIVE[1], out=rec, record_ld=ld,
                       status=st, outputs=tuple(lists), **kw)
        c.sync()
        assert hip.stream_query(stream) == sh.HIP_SUCCESS
        streams = c.profile_streams()
        c.profile(False)
        c.free_host(pinned)
        assert streams.get("unpack_pcm24") == 0 and streams.get("host_rows") == 0 and streams.get("pitch_path_write") == 0, streams
        got = (rec.numpy(), st.numpy()) + tuple(d.numpy() for d in lists)
        _assert_same("own stream", got, want, width)
        # no state is left for a stitch
        assert c.L.vbx_track_stitch_f64(c.ctx, rec.ptr + 16, F, ld, 1, F, rec.ptr + 16, None) == E_INVALID
    finally:
        c.sync()
        c.close()
        hip.stream_sync(stream)
        hip.stream_destroy(stream)


# ---- 5. layouts and errors -----------------------------------------------------------------------------------------------------------

def test_outputs_fenced(vb, pkg, base):
    """Padded record rows, all four list outputs the caller's: nothing outside them is written."""
    form, width = "tracked_ext", _width(vb, pkg, "tracked_ext")
    a, kw, _, _ = _recording(base, "pcm32_3ch2", *NATIVE)
    want = _resident(vb, pkg, base, "pcm32_3ch2", NATIVE, form, SEG5)
    ext, track = _form(pkg, form)
    ld = width + (width & 1) + 6
    ar = la.Arena(la.DeviceBackend(vb), "analyze_host fenced")
    ar.output("records", np.float64, F, width, ld=ld)
    ar.output("status3", np.int32, 3, F)
    ar.output("count", np.int32, 1, F)
    ar.output("peak", np.float64, 1, F)
    ar.output("index", np.int32, 1, F)
    ar.place()
    outputs = pkg.PitchTrackOutputs(None, ar["count"], ar["peak"], ar["index"])
    assert vb.analyze_host(a, _params(pkg), ext, track, chunk_frames=200, seg_start=SEG5, frame_len=NATIVE[0], stride=NATIVE[1],
                           out=ar["records"], record_ld=ld, status=ar["status3"], outputs=outputs, **kw) is None
    out = ar.finish()
    la.assert_same_bits(ar.label, "records", out["records"], want[0][:, :width])
    la.assert_same_bits(ar.label, "status3", out["status3"], want[1])
    la.assert_same_bits(ar.label, "count", out["count"][0], want[3])
    la.assert_same_bits(ar.label, "peak", out["peak"][0], want[4])
    la.assert_same_bits(ar.label, "index", out["index"][0], want[5])


def test_errors_leave_the_outputs_untouched(vb, pkg, base):
    N, H = NATIVE
    a, _, chan, _ = _recording(base, "pcm16", N, H)
    params = _params(pkg)
    ext, track = _form(pkg, "tracked_ext")
    width = _width(vb, pkg, "tracked_ext")
    ld = width + (width & 1)
    fn = vb.L.vbx_analyze_host
    ar = la.Arena(la.DeviceBackend(vb), "analyze_host errors")
    ar.output("records", np.float64, F, ld)
    ar.output("at8", np.float64, F, ld, residue=8)
    ar.output("status3", np.int32, 3, F)
    ar.output("cand", np.float64, F, 8)
    ar.output("count", np.int32, 1, F)
    ar.output("peak", np.float64, 1, F)
    ar.output("index", np.int32, 1, F)
    ar.place()
    outs = pkg.PitchTrackOutputs(ar["cand"], ar["count"], ar["peak"], ar["index"])
    seg = np.array(SEG5, dtype=np.int64)

    def call(audio=a.ctypes.data, n=a.size, hf=None, no_fmt=False, frame_len=N, p=params, e=ext, t=track, sg=seg, records=None, rld=ld):
        hf = pkg.HostAudio.make(1, 1, 0, 200) if hf is None else hf
        return fn(vb.ctx, audio, n, None if no_fmt else C.byref(hf), frame_len, H, C.byref(p), None if e is None else C.byref(e),
                  None if t is None else C.byref(t), None if sg is None else sg.ctypes.data, 0 if sg is None else sg.size,
                  ar["records"] if records is None else records, rld, ar["status3"], C.byref(outs))

    def fmt(format=1, channels=1, channel=0, reserved=0, chunk=200):
        h = pkg.HostAudio.make(format, channels, channel, chunk)
        h.reserved = reserved
        return h
    assert call(no_fmt=True) == E_INVALID
    for bad in (fmt(format=0), fmt(format=6), fmt(channels=0), fmt(channels=2, channel=2), fmt(channel=-1), fmt(reserved=1),
                fmt(chunk=1), fmt(chunk=63)):
        assert call(hf=bad) == E_INVALID, (bad.format, bad.channels, bad.channel, bad.reserved, bad.chunk_frames)
    assert call(audio=None) == E_INVALID                       # a NULL recording with frames to read
    # what the resident call rejects
    assert call(rld=ld + 1) == E_INVALID and call(rld=width - 2) == E_INVALID
    assert call(records=ar["at8"]) == E_INVALID
    assert call(e=pkg.AnalysisExt.make(-1.0)) == E_INVALID
    assert call(t=pkg.PitchTrackParams.make(kmax=0)) == E_INVALID and call(t=pkg.PitchTrackParams.make(kmax=64)) == E_INVALID
    assert call(sg=np.array([1, 5], dtype=np.int64)) == E_INVALID and call(sg=np.array([0, F + 1], dtype=np.int64)) == E_INVALID
    assert call(p=_params(pkg, mfcc=(65, 100.0, 8000.0))) == E_INVALID
    assert call(p=_params(pkg, mfcc=(65, 100.0, 8000.0)), e=None, t=None) == E_INVALID
    assert call(p=_params(pkg, formant_order=63)) == E_INVALID
    # the empty recording succeeds: fewer samples than one frame, NULL pointers
    assert call(n=N - 1, sg=None) == 0 and call(audio=None, n=0, sg=None) == 0
    assert fn(vb.ctx, None, 100, C.byref(fmt()), N, H, C.byref(params), None, None, None, 0, None, ld, None, None) == 0
    out = ar.finish()
    for name, arr in out.items():
        assert la.unwritten(arr).shape[0] == arr.size, name
    # the context is usable afterwards
    _assert_same("after the errors", _host(vb, pkg, base, "pcm16", NATIVE, "tracked_ext", SEG5, 200),
                 _resident(vb, pkg, base, "pcm16", NATIVE, "tracked_ext", SEG5), width)
