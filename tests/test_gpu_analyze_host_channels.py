"""vbx_analyze_host_channels on a real MI355X: several channels of a host-resident recording from ONE upload per chunk, against
vbx_analyze_host on each channel (which tests/test_gpu_analyze_host.py holds to the resident call).  Every output is compared BIT
FOR BIT (uint64 views): the records, the three status rows and, tracked, the candidate lists, counts, peaks and path indices.
F = 400 frames: at chunk_frames 64 seven chunks, at 150 a ragged last chunk of 100, at 400 one chunk.  Segments [0, 150, 230, 300]:
at chunk_frames 150 the starts 150 and 300 lie on a cut and 230 inside a chunk; at 64 all lie inside chunks.  The channels are
derived from one recording -- rolled, reversed, scaled sums -- so that no two agree."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import layout_arena as la
import stream_harness as sh

pytestmark = pytest.mark.gpu

SR = 48000.0
F = 400
NATIVE, WIDENED = (1200, 480), (1024, 512)
SEG4 = [0, 150, 230, 300]
E_INVALID = -1
FORMATS = ["pcm16", "pcm24", "pcm32", "f32", "f64"]
FORMAT_CODE = {"pcm16": 1, "pcm24": 2, "pcm32": 3, "f32": 4, "f64": 5}


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _params(pkg, **kw):
    kw.setdefault("est_init", np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES]))
    return pkg.AnalysisParams.make(SR, **kw)


def _form(pkg, form):
    """(ext, track) of a form: ext = find_formants at ratio 0.25 plus the RMS column; track = kmax 4 with the default costs"""
    ext = pkg.AnalysisExt.make(0.25, rms=True) if "ext" in form else None
    track = pkg.PitchTrackParams.make(kmax=4) if "tracked" in form else None
    return ext, track


def _width(vb, pkg, form):
    ext, _ = _form(pkg, form)
    p = _params(pkg)
    return int(vb.L.vbx_record_doubles_ex(C.byref(p), None if ext is None else C.byref(ext)))


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
    x[90_000:90_000 + m] = pcm[:m].astype(np.float64) / 32767.0
    return x


def _pack24(s):
    return np.ascontiguousarray(np.ascontiguousarray(s, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)


_REC = {}


def _recording(base, fmt, channels, shape):
    """(host audio as the calls take it, the keyword arguments that describe it)"""
    key = (fmt, channels, shape)
    if key not in _REC:
        N, H = shape
        x = base[:(F - 1) * H + N] * 0.9
        other = np.roll(x, 777)[::-1].copy()
        cols = [x, other] + [(0.55 - 0.05 * j) * np.roll(x, 313 * j) + (0.2 + 0.03 * j) * np.roll(other, 1009 * j) for j in range(1, 7)]
        y = np.stack(cols[:channels], axis=1)
        if fmt == "pcm16":
            _REC[key] = np.ascontiguousarray(np.round(y * 32767.0).astype(np.int16)), {}
        elif fmt == "pcm24":
            _REC[key] = _pack24(np.round(y * 8388607.0).astype(np.int32).reshape(-1)), dict(format=2, channels=channels)
        elif fmt == "pcm32":
            _REC[key] = np.ascontiguousarray(np.round(y * 2147483647.0).astype(np.int64).astype(np.int32)), {}
        elif fmt == "f32":
            _REC[key] = np.ascontiguousarray(y.astype(np.float32)), {}
        else:
            _REC[key] = np.ascontiguousarray(y), {}
    return _REC[key]


_REF = {}


def _single(vb, pkg, base, fmt, channels, channel, shape, form, seg, chunk, policy="EXACT"):
    """vbx_analyze_host on one channel, computed once per case"""
    key = (fmt, channels, channel, shape, form, None if seg is None else tuple(seg), chunk, policy)
    if key not in _REF:
        a, kw = _recording(base, fmt, channels, shape)
        ext, track = _form(pkg, form)
        _REF[key] = vb.analyze_host(a, _params(pkg), ext, track, channel=channel, chunk_frames=chunk, seg_start=seg, frame_len=shape[0],
                                    stride=shape[1], lists=track is not None, **kw)
    return _REF[key]


def _multi(vb, pkg, base, fmt, channels, select, shape, form, seg, chunk, audio=None, lists=None):
    a, kw = _recording(base, fmt, channels, shape)
    ext, track = _form(pkg, form)
    return vb.analyze_host_channels(a if audio is None else audio, _params(pkg), ext, track, select=select, chunk_frames=chunk,
                                    seg_start=seg, frame_len=shape[0], stride=shape[1],
                                    lists=(track is not None) if lists is None else lists, **kw)


def _assert_same(label, got, want, width):
    rec, st = got[0][:, :width], got[1]
    wrec, wst = want[0][:, :width], want[1]
    assert rec.shape == wrec.shape == (F, width), (label, rec.shape, wrec.shape)
    a, b = _u64(rec), _u64(wrec)
    assert np.array_equal(a, b), (label, "records: first differing (frame, column)", tuple(np.argwhere(a != b)[0]), int((a != b).sum()))
    assert np.array_equal(st, wst), (label, "status3", np.argwhere(st != wst)[:8])
    if len(got) > 2:
        cand, count, peak, index = got[2:]
        wcand, wcount, wpeak, windex = want[2:]
        assert np.array_equal(count, wcount), (label, "count", np.argwhere(count != wcount)[:8])
        assert np.array_equal(index, windex), (label, "index", np.argwhere(index != windex)[:8])
        assert np.array_equal(_u64(peak), _u64(wpeak)), (label, "peak", np.argwhere(_u64(peak) != _u64(wpeak))[:8])
        keep = np.arange(cand.shape[1])[None, :] < count[:, None]             # (entries past a frame's count are not written)
        assert np.array_equal(_u64(cand)[keep], _u64(wcand)[keep]), (label, "candidate lists")


def _check(vb, pkg, base, fmt, channels, select, shape, form, seg, chunk, policy="EXACT", audio=None):
    sel = list(range(channels)) if select is None else list(select)
    got = _multi(vb, pkg, base, fmt, channels, select, shape, form, seg, chunk, audio=audio)
    assert len(got) == len(sel)
    for k, c in enumerate(sel):
        want = _single(vb, pkg, base, fmt, channels, c, shape, form, seg, chunk, policy)
        assert len(got[k]) == len(want)
        _assert_same(f"{fmt} x{channels} selection {sel} entry {k} (channel {c}) {shape} {form} seg {seg} chunk {chunk} {policy}",
                     got[k], want, _width(vb, pkg, form))
    return got


@pytest.fixture
def policy(vb, pkg):
    old = vb.lpc_policy

    def set_policy(name):
        vb.lpc_policy = getattr(pkg, "LPC_POLICY_" + name)
    yield set_policy
    vb.lpc_policy = old


# ---- 1. formats, channel counts, selections ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [NATIVE, WIDENED], ids=["1200/480", "1024/512"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_three_channels(vb, pkg, base, fmt, shape):
    _check(vb, pkg, base, fmt, 3, None, shape, "tracked_ext", SEG4, 150)
    _check(vb, pkg, base, fmt, 3, None, shape, "plain", None, 64)


@pytest.mark.parametrize("channels,select", [(2, [1, 0]), (8, [6, 3, 1])], ids=["stereo reversed", "three of eight reversed"])
def test_pcm16_reversed_subsets(vb, pkg, base, channels, select):
    for shape in (NATIVE, WIDENED):
        _check(vb, pkg, base, "pcm16", channels, select, shape, "tracked_ext", SEG4, 150)


def test_one_channel_is_analyze_host(vb, pkg, base):
    for fmt in FORMATS:                                        # (PCM16, F32 and F64: the slot is read as it is)
        _check(vb, pkg, base, fmt, 1, None, NATIVE, "tracked_ext", SEG4, 150)
    _check(vb, pkg, base, "pcm24", 1, [0], WIDENED, "plain", None, 64)


# ---- 2. forms, cuts, segment lists, policies --------------------------------------------------------------------------------------

@pytest.mark.parametrize("seg", [None, SEG4], ids=["one utterance", "four utterances"])
@pytest.mark.parametrize("form", ["plain", "tracked", "ext", "tracked_ext"])
def test_every_cut_and_form(vb, pkg, base, form, seg):
    for chunk in (64, 150, 400):
        _check(vb, pkg, base, "pcm16", 2, None, NATIVE, form, seg, chunk)
    _check(vb, pkg, base, "pcm24", 2, [1, 0], WIDENED, form, seg, 150)


@pytest.mark.parametrize("form", ["tracked", "tracked_ext"])
def test_tracked_without_the_callers_lists(vb, pkg, base, form):
    """No outputs structure at all: the lists, counts, peaks and status rows of every channel live in the context workspace, and
    the records -- columns 0-1 are the path -- are the same."""
    for seg, chunk in ((SEG4, 64), (None, 150)):
        got = _multi(vb, pkg, base, "f32", 3, [2, 0, 1], NATIVE, form, seg, chunk, lists=False)
        for k, c in enumerate([2, 0, 1]):
            assert len(got[k]) == 2
            _assert_same(f"{form} without lists, channel {c}, chunk {chunk}", got[k],
                         _single(vb, pkg, base, "f32", 3, c, NATIVE, form, seg, chunk)[:2], _width(vb, pkg, form))


@pytest.mark.parametrize("pol", ["EXACT", "REFERENCE"])
def test_lpc_policies(vb, pkg, base, policy, pol):
    policy(pol)
    for fmt in ("pcm16", "pcm32"):
        _check(vb, pkg, base, fmt, 2, None, NATIVE, "tracked_ext", SEG4, 150, pol)
        _check(vb, pkg, base, fmt, 2, None, NATIVE, "plain", None, 64, pol)


# ---- 3. what runs -------------------------------------------------------------------------------------------------------------------

def _profiled(vb, call):
    vb.profile(True)
    vb.profile_reset()
    try:
        call()
        return vb.profile_report(), vb.profile_streams()
    finally:
        vb.profile(False)


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_unpack_launch_per_chunk(vb, pkg, base, fmt):
    """Three channels, four chunks: four unpack_all launches on the context's stream, none of the per-channel kernel; twelve copies
    of rows and nine stitches (every channel at every cut)."""
    rep, streams = _profiled(vb, lambda: _multi(vb, pkg, base, fmt, 3, None, NATIVE, "plain", None, 100))
    name = "unpack_all_" + fmt
    assert rep.get(name, (0, 0))[1] == 4 and streams[name] == 0, sorted(rep)
    assert [n for n in rep if n.startswith("unpack_")] == [name], sorted(rep)
    assert rep["host_rows"][1] == 12 and rep["tracker_stitch"][1] == 9, sorted(rep)


def test_native_stays_native(vb, pkg, base):
    """Stereo PCM16 and float32 at 1200 / 480: every plane is read as a resident recording would be -- no widening pass."""
    for fmt in ("pcm16", "f32"):
        rep, _ = _profiled(vb, lambda: _multi(vb, pkg, base, fmt, 2, None, NATIVE, "tracked_ext", SEG4, 100))
        assert rep["host_rows"][1] == 8 and rep["unpack_all_" + fmt][1] == 4, sorted(rep)
        assert [n for n in rep if n.startswith("unpack_")] == ["unpack_all_" + fmt], sorted(rep)      # no per-channel unpack launch
        for name in rep:
            assert name not in ("pcm16", "f32_to_f64"), (fmt, name, sorted(rep))


# ---- 4. host memory and ordering ----------------------------------------------------------------------------------------------------

def test_pinned_and_pageable_memory_give_the_same_bits(vb, pkg, base):
    for fmt in ("pcm16", "pcm24"):
        a, _ = _recording(base, fmt, 3, NATIVE)
        pinned = vb.malloc_host(a.shape, a.dtype)
        pinned[...] = a
        _check(vb, pkg, base, fmt, 3, [2, 1, 0], NATIVE, "tracked_ext", SEG4, 150, audio=pinned)
        _check(vb, pkg, base, fmt, 3, [2, 1, 0], NATIVE, "tracked_ext", SEG4, 150)
        vb.free_host(pinned)


def _device_outputs(vb, n_sel, ld):
    """per channel: records, status rows, and the four list outputs at kmax 4"""
    return [[vb.empty((F, ld)), vb.empty((3, F), np.int32), vb.empty((F, 4, 2)), vb.empty(F, np.int32), vb.empty(F), vb.empty(F, np.int32)]
            for _ in range(n_sel)]


def _queue(vb, pkg, audio, sel, outs, ld, chunk, seg, **kw):
    ext, track = _form(pkg, "tracked_ext")
    assert vb.analyze_host_channels(audio, _params(pkg), ext, track, select=sel, chunk_frames=chunk, seg_start=seg, frame_len=NATIVE[0],
                                    stride=NATIVE[1], out=[o[0] for o in outs], record_ld=ld, status=[o[1] for o in outs],
                                    outputs=[tuple(o[2:]) for o in outs], **kw) is None


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_the_audio_may_be_overwritten_when_the_call_returns(vb, pkg, base, pinned):
    width = _width(vb, pkg, "tracked_ext")
    ld = width + (width & 1)
    a, kw = _recording(base, "pcm16", 2, NATIVE)
    want = [_single(vb, pkg, base, "pcm16", 2, c, NATIVE, "tracked_ext", SEG4, 64) for c in (0, 1)]
    buf = vb.malloc_host(a.shape, a.dtype) if pinned else np.empty_like(a)
    buf[...] = a
    outs = _device_outputs(vb, 2, ld)
    vb.sync()
    _queue(vb, pkg, buf, [0, 1], outs, ld, 64, SEG4, **kw)
    buf[...] = -12345                                          # no wait in between
    for k in range(2):
        _assert_same(f"audio overwritten on return, channel {k}", tuple(d.numpy() for d in outs[k]), want[k], width)
    for d in sum(outs, []):
        d.free()
    if pinned:
        vb.free_host(buf)


def test_two_calls_back_to_back_without_a_wait(vb, pkg, base):
    """A delay keeps the stream busy, then two calls on two different stereo buffers follow with no wait between them (two chunks
    each, one utterance: nothing makes the host wait for the device): the second call's uploads must wait for the first call's
    readers of the staging slots."""
    width = _width(vb, pkg, "tracked_ext")
    ld = width + (width & 1)
    a, kw = _recording(base, "pcm16", 2, NATIVE)
    swapped = np.ascontiguousarray(a[:, ::-1])
    want = [_single(vb, pkg, base, "pcm16", 2, c, NATIVE, "tracked_ext", None, 200) for c in (0, 1)]
    _multi(vb, pkg, base, "pcm16", 2, None, NATIVE, "tracked_ext", None, 200)      # (sizes the workspaces, outside the queue)
    pinned = []
    for src in (a, swapped):
        pinned.append(vb.malloc_host(src.shape, src.dtype))
        pinned[-1][...] = src
    outs = [_device_outputs(vb, 2, ld) for _ in range(2)]
    delay = sh.Delay(vb, pkg)
    reps = delay.reps_for(1.0)
    vb.sync()
    assert delay.timed(reps) >= sh.DELAY_MIN_MS                  # (else the test is vacuous)
    delay.queue(reps)
    for buf, o in zip(pinned, outs):
        _queue(vb, pkg, buf, [0, 1], o, ld, 200, None, **kw)
    vb.sync()
    for call, order in enumerate(((0, 1), (1, 0))):              # the second buffer holds the channels swapped
        for k, c in enumerate(order):
            _assert_same(f"call {call} of two queued back to back, entry {k}", tuple(d.numpy() for d in outs[call][k]), want[c], width)
    for d in sum(sum(outs, []), []):
        d.free()
    for b in pinned:
        vb.free_host(b)


def test_sync_leaves_nothing_running(pkg, base):
    """A context on a caller-created stream: after vbx_sync that stream is idle, the pinned recording and every output can be freed,
    every new launch ran on the context's stream, and no state is left for a stitch."""
    hip = sh.Hip(pkg)
    stream = hip.stream_create()
    c = pkg.VoxBox(0, stream)
    try:
        a, kw = _recording(base, "pcm24", 2, NATIVE)
        ext, track = _form(pkg, "tracked_ext")
        p = _params(pkg)
        width = int(c.L.vbx_record_doubles_ex(C.byref(p), C.byref(ext)))
        ld = width + (width & 1)
        want = [c.analyze_host(a, p, ext, track, channel=ch, chunk_frames=150, seg_start=SEG4, frame_len=NATIVE[0], stride=NATIVE[1],
                               lists=True, **kw) for ch in (0, 1)]
        pinned = c.malloc_host(a.shape, a.dtype)
        pinned[...] = a
        outs = _device_outputs(c, 2, ld)
        c.profile(True)
        c.profile_reset()
        _queue(c, pkg, pinned, [0, 1], outs, ld, 150, SEG4, **kw)
        c.sync()
        assert hip.stream_query(stream) == sh.HIP_SUCCESS
        streams = c.profile_streams()
        c.profile(False)
        c.free_host(pinned)
        assert streams.get("unpack_all_pcm24") == 0 and streams.get("host_rows") == 0 and streams.get("pitch_path_write") == 0, streams
        for k in range(2):
            _assert_same(f"own stream, channel {k}", tuple(d.numpy() for d in outs[k]), want[k], width)
        rec = outs[1][0]
        assert c.L.vbx_track_stitch_f64(c.ctx, rec.ptr + 16, F, ld, 1, F, rec.ptr + 16, None) == E_INVALID
    finally:
        c.sync()
        c.close()
        hip.stream_sync(stream)
        hip.stream_destroy(stream)


# ---- 5. layouts and errors ------------------------------------------------------------------------------------------------------------

def test_outputs_fenced(vb, pkg, base):
    """Padded record rows in fenced arenas, the list outputs the caller's: nothing outside them is written."""
    form, width = "tracked_ext", _width(vb, pkg, "tracked_ext")
    a, kw = _recording(base, "pcm32", 3, NATIVE)
    sel = [2, 0]
    want = [_single(vb, pkg, base, "pcm32", 3, c, NATIVE, form, SEG4, 150) for c in sel]
    ld = width + (width & 1) + 6
    ar = la.Arena(la.DeviceBackend(vb), "analyze_host_channels fenced")
    for k in range(2):
        ar.output(f"records{k}", np.float64, F, width, ld=ld)
        ar.output(f"status3{k}", np.int32, 3, F)
        ar.output(f"count{k}", np.int32, 1, F)
        ar.output(f"peak{k}", np.float64, 1, F)
        ar.output(f"index{k}", np.int32, 1, F)
    ar.place()
    ext, track = _form(pkg, form)
    outputs = [pkg.PitchTrackOutputs(None, ar[f"count{k}"], ar[f"peak{k}"], ar[f"index{k}"]) for k in range(2)]
    assert vb.analyze_host_channels(a, _params(pkg), ext, track, select=sel, chunk_frames=150, seg_start=SEG4, frame_len=NATIVE[0],
                                    stride=NATIVE[1], out=[ar["records0"], ar["records1"]], record_ld=ld,
                                    status=[ar["status30"], ar["status31"]], outputs=outputs, **kw) is None
    out = ar.finish()
    for k in range(2):
        la.assert_same_bits(ar.label, f"records{k}", out[f"records{k}"], want[k][0][:, :width])
        la.assert_same_bits(ar.label, f"status3{k}", out[f"status3{k}"], want[k][1])
        la.assert_same_bits(ar.label, f"count{k}", out[f"count{k}"][0], want[k][3])
        la.assert_same_bits(ar.label, f"peak{k}", out[f"peak{k}"][0], want[k][4])
        la.assert_same_bits(ar.label, f"index{k}", out[f"index{k}"][0], want[k][5])


def test_errors_leave_the_outputs_untouched(vb, pkg, base):
    N, H = NATIVE
    a, _ = _recording(base, "pcm16", 2, NATIVE)
    params = _params(pkg)
    ext, track = _form(pkg, "tracked_ext")
    width = _width(vb, pkg, "tracked_ext")
    ld = width + (width & 1)
    fn = vb.L.vbx_analyze_host_channels
    ar = la.Arena(la.DeviceBackend(vb), "analyze_host_channels errors")
    ar.output("records", np.float64, 2 * F, ld)                # two channels' records, one behind the other
    ar.output("at8", np.float64, F, ld, residue=8)
    ar.output("status3", np.int32, 6, F)
    ar.output("count", np.int32, 2, F)
    ar.output("index", np.int32, 2, F)
    ar.place()
    seg = np.array(SEG4, dtype=np.int64)
    r0, r1 = ar["records"], ar["records"] + F * ld * 8
    pto = [pkg.PitchTrackOutputs(None, ar["count"] + 4 * F * k, None, ar["index"] + 4 * F * k) for k in range(2)]

    def entries(recs=(r0, r1)):
        e = (pkg.ChannelOutputs * 2)()
        for k in range(2):
            e[k].records, e[k].status3, e[k].outputs = recs[k], ar["status3"] + 12 * F * k, C.pointer(pto[k])
        return e

    def call(audio=a.ctypes.data, n=a.shape[0], hf=None, no_fmt=False, sel=(0, 1), n_sel=None, no_sel=False, frame_len=N, p=params, e=ext,
             t=track, sg=seg, out=None, no_out=False, rld=ld):
        hf = pkg.HostAudio.make(1, 2, 0, 150) if hf is None else hf
        s = np.array(sel, dtype=np.int32)
        out = entries() if out is None else out
        return fn(vb.ctx, audio, n, None if no_fmt else C.byref(hf), None if no_sel else s.ctypes.data, len(sel) if n_sel is None else n_sel,
                  frame_len, H, C.byref(p), None if e is None else C.byref(e), None if t is None else C.byref(t),
                  None if sg is None else sg.ctypes.data, 0 if sg is None else sg.size, None if no_out else out, rld)

    def fmt(format=1, channels=2, channel=0, reserved=0, chunk=150):
        h = pkg.HostAudio.make(format, channels, channel, chunk)
        h.reserved = reserved
        return h
    # what vbx_analyze_host rejects
    assert call(no_fmt=True) == E_INVALID
    for bad in (fmt(format=0), fmt(format=6), fmt(channels=0), fmt(reserved=1), fmt(chunk=1), fmt(chunk=63)):
        assert call(hf=bad) == E_INVALID, (bad.format, bad.channels, bad.channel, bad.reserved, bad.chunk_frames)
    assert call(audio=None) == E_INVALID
    assert call(rld=ld + 1) == E_INVALID and call(rld=width - 2) == E_INVALID
    assert call(e=pkg.AnalysisExt.make(-1.0)) == E_INVALID
    assert call(t=pkg.PitchTrackParams.make(kmax=0)) == E_INVALID and call(t=pkg.PitchTrackParams.make(kmax=64)) == E_INVALID
    assert call(sg=np.array([1, 5], dtype=np.int64)) == E_INVALID and call(sg=np.array([0, F + 1], dtype=np.int64)) == E_INVALID
    assert call(p=_params(pkg, mfcc=(65, 100.0, 8000.0))) == E_INVALID
    assert call(p=_params(pkg, formant_order=63)) == E_INVALID
    # the call's own: the channel field, the selection, the entries
    assert call(hf=fmt(channel=1)) == E_INVALID and call(hf=fmt(channel=-1)) == E_INVALID
    assert call(no_sel=True) == E_INVALID and call(n_sel=0) == E_INVALID and call(sel=(0, 1, 0), n_sel=3) == E_INVALID
    assert call(sel=(1, 1)) == E_INVALID and call(sel=(0, 2)) == E_INVALID and call(sel=(-1, 0)) == E_INVALID
    assert call(hf=fmt(channels=1), sel=(0, 0)) == E_INVALID
    assert call(no_out=True) == E_INVALID
    assert call(out=entries((r0, None))) == E_INVALID and call(out=entries((None, r1))) == E_INVALID
    assert call(out=entries((r0, ar["at8"]))) == E_INVALID
    assert call(out=entries((r0, r0))) == E_INVALID and call(out=entries((r0, r0 + 16 * ld))) == E_INVALID      # overlapping records
    assert call(out=entries((r1, r1 - 8 * ld))) == E_INVALID
    # the empty recording succeeds: fewer samples than one frame, NULL pointers
    assert call(n=N - 1, sg=None) == 0 and call(audio=None, n=0, sg=None) == 0
    out = ar.finish(free=False)
    for name, arr in out.items():
        assert la.unwritten(arr).shape[0] == arr.size, name
    # the next valid call on the same context succeeds, and its outputs are the single-channel calls'
    assert call() == 0
    out = ar.finish()
    for k in range(2):
        want = _single(vb, pkg, base, "pcm16", 2, k, NATIVE, "tracked_ext", SEG4, 150)
        la.assert_same_bits("after the errors", f"records {k}", out["records"][k * F:(k + 1) * F, :width], want[0][:, :width])
        la.assert_same_bits("after the errors", f"status3 {k}", out["status3"][3 * k:3 * k + 3], want[1])
        la.assert_same_bits("after the errors", f"index {k}", out["index"][k], want[5])
