"""A live session (vbx_session_*) on a real MI355X: the recording of tests/test_gpu_analyze_host.py (synthetic speech with a stretch
of the golden 16-bit WAV), F = 200 frames, pushed block by block in every way the header promises, against the RESIDENT call on the
whole recording -- vbx_analyze_frames_ex_pcm16 for PCM16, _f32in for float32, _f64 on the converted samples for 24- / 32-bit PCM and
double.  Nothing is compared with a tolerance: every frame of the records, the three status rows and, tracked, the candidate lists,
counts and peaks is compared on uint64 / integer views, and the tracked contour is vbx_pitch_path_f64 over the accumulated lists
against the resident tracked call's columns 0-1 and indices.  References are computed once per key."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import layout_arena as la
import stream_harness as sh
import test_gpu_analyze_host as ah

pytestmark = pytest.mark.gpu

SR = 48000.0
F = 200
NATIVE, WIDENED = (1200, 480), (1024, 512)
E_INVALID = -1
KMAX = 4
FMT_OF_DTYPE = {np.dtype(np.int16): 1, np.dtype(np.int32): 3, np.dtype(np.float32): 4, np.dtype(np.float64): 5}
SRC_BYTES = {1: 2, 2: 3, 3: 4, 4: 4, 5: 8}
_u64 = ah._u64


@pytest.fixture(scope="module")
def base(vb, golden_dir):
    """the recording as doubles in (-1, 1): the synthetic speech with a stretch of the golden 16-bit WAV inside the 200 frames"""
    n = (F - 1) * 1000 + 1200
    d = vb.synth_speech(n, sample_offset=5 * 48000 + 321)
    x = d.numpy()
    d.free()
    with wave.open(os.path.join(golden_dir, "sample-two_vowels.wav"), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    m = min(pcm.size, 40_000)
    x[30_000:30_000 + m] = pcm[:m].astype(np.float64) / 32767.0
    return x


_REC, _REF = {}, {}


def _recording(base, fmt, N, H):
    """(host audio, format code, channels, channel, the selected channel for the resident call, which resident call)"""
    if (fmt, N, H) not in _REC:
        audio, kw, chan, which = ah._make_recording(base[:(F - 1) * H + N], fmt, N, H)
        code = kw.get("format") or FMT_OF_DTYPE[audio.dtype]
        channels = audio.shape[1] if audio.ndim == 2 else 1
        _REC[(fmt, N, H)] = (audio, code, channels, kw.get("channel", 0), chan, which)
    return _REC[(fmt, N, H)]


def _reference(vb, pkg, chan, which, shape, form, seg=None, key=None):
    """the resident call's outputs on the selected channel: (records, status3[, cand, count, peak, index])"""
    if key is None or key not in _REF:
        N, H = shape
        ext, track = ah._form(pkg, form)
        fn = {"pcm16": vb.analyze_frames_ex_pcm16, "f32in": vb.analyze_frames_ex_f32in, "f64": vb.analyze_frames_ex}[which]
        got = fn(chan, ah._params(pkg), ext, track, seg_start=seg, frame_len=N, stride=H, n_frames=F, lists=track is not None)
        if key is None:
            return got
        _REF[key] = got
    return _REF[key]


def _resident(vb, pkg, base, fmt, shape, form, seg=None, policy="EXACT"):
    _, _, _, _, chan, which = _recording(base, fmt, *shape)
    return _reference(vb, pkg, chan, which, shape, form, seg, key=(fmt, shape, form, None if seg is None else tuple(seg), policy))


def _block(audio, code, a, b):
    """sample frames [a, b) of the host audio"""
    return audio[3 * a:3 * b] if code == 2 else audio[a:b]


class Outputs:
    """one global set of device outputs for F frames, canary-filled; a push writes its rows at their global offsets"""

    def __init__(self, vb, pkg, form, n_frames=F):
        self.vb, self.F = vb, n_frames
        self.width = ah._width(vb, pkg, form)
        self.ld = self.width + (self.width & 1)
        self.tracked = "tracked" in form
        self.rec, self.st = vb.empty((n_frames, self.ld)), vb.empty((3, n_frames), np.int32)
        self.lists = [vb.empty((n_frames, KMAX, 2)), vb.empty(n_frames, np.int32), vb.empty(n_frames)] if self.tracked else []
        for d in [self.rec, self.st] + self.lists:
            vb._check(vb.L.vbx_memset(vb.ctx, d.ptr, 0xFF, d.nbytes))

    def at(self, lo):
        """(out, status, outputs, record_ld, status_ld) of a push whose first frame is lo"""
        outs = None
        if self.tracked:
            outs = (self.lists[0].ptr + lo * KMAX * 16, self.lists[1].ptr + lo * 4, self.lists[2].ptr + lo * 8, None)
        return dict(out=self.rec.ptr + lo * self.ld * 8, status=self.st.ptr + lo * 4, outputs=outs, record_ld=self.ld, status_ld=self.F)

    def download(self):
        got = (self.rec.numpy(), self.st.numpy()) + tuple(d.numpy() for d in self.lists)
        return got

    def free(self):
        for d in [self.rec, self.st] + self.lists:
            d.free()


def _feed(sess, o, audio, code, sizes, marks=(), start=0, between=None, pusher=None):
    """pushes the blocks of `sizes` from sample frame `start` on; an utterance is marked wherever the frames delivered reach a mark"""
    pos, c0 = start, sess.info()[0]
    for i, n in enumerate(sizes):
        lo = sess.info()[1]
        if lo in marks:
            sess.mark_utterance()                                            # (again after a push without a frame: the same frame index)
        want_n = sess.frames_of(n)
        if pusher is None:
            assert sess.push(_block(audio, code, pos, pos + n), **o.at(lo)) is None
        else:
            pusher(sess, pos, n, o.at(lo))
        pos += n
        assert sess.info()[:2] == (c0 + pos - start, lo + want_n)
        if between is not None:
            between(i)
    return pos


def _assert_session(label, vb, pkg, o, want, shape, form, seg=None):
    """every frame, bit for bit: the records (tracked: from column 2, columns 0-1 still the canary), the status rows, the lists; and,
    tracked, vbx_pitch_path_f64 over the accumulated lists against the resident call's columns 0-1 and indices"""
    got = o.download()
    c0 = 2 if o.tracked else 0
    a, b = _u64(got[0][:, c0:o.width]), _u64(want[0][:, c0:o.width])
    assert a.shape == b.shape == (F, o.width - c0), (label, a.shape, b.shape)
    assert np.array_equal(a, b), (label, "records: first differing (frame, column)", tuple(np.argwhere(a != b)[0]), int((a != b).sum()))
    assert np.array_equal(got[1], want[1]), (label, "status3", np.argwhere(got[1] != want[1])[:8])
    if o.tracked:
        assert np.all(_u64(got[0][:, :2]) == 0xFFFFFFFFFFFFFFFF), (label, "columns 0-1 were written")
        cand, count, peak = got[2:]
        wcand, wcount, wpeak, windex = want[2:]
        assert np.array_equal(count, wcount), (label, "count", np.argwhere(count != wcount)[:8])
        assert np.array_equal(_u64(peak), _u64(wpeak)), (label, "peak", np.argwhere(_u64(peak) != _u64(wpeak))[:8])
        keep = np.arange(cand.shape[1])[None, :] < count[:, None]
        assert np.array_equal(_u64(cand)[keep], _u64(wcand)[keep]), (label, "candidate lists")
        _, track = ah._form(pkg, form)
        path = pkg.PitchPathParams.from_buffer_copy(track.path)
        path.time_step = shape[1] / SR                                      # the batch's own hop, as the tracked call sets it
        st_pitch = vb.to_device(got[1][0])
        contour, index = vb.pitch_path(o.lists[0], o.lists[1], status=st_pitch, local_peak=o.lists[2], seg_start=seg, params=path,
                                       n_frames=F, kmax=KMAX)
        st_pitch.free()
        pa, pb = _u64(contour), _u64(want[0][:, :2])
        assert np.array_equal(pa, pb), (label, "the path over the pushed lists", tuple(np.argwhere(pa != pb)[0]), int((pa != pb).sum()))
        assert np.array_equal(index, windex), (label, "path indices", np.argwhere(index != windex)[:8])


def _schedule(name, N, H, seed=7):
    T = (F - 1) * H + N
    if name == "one":
        return [T]
    if name == "hop":
        return [N] + [H] * (F - 1)
    rng = np.random.default_rng(seed)
    if name == "ragged":
        # a first cut with more than 64 frames before it (warm = 64, the stitch runs), sizes in [1, 3 H], two blocks of 60 - 70 hops
        # (64.5 + 61 + 61 + 4 x 3 hops at most: the recording's 199 hops hold all of them whole)
        sizes = [N + 64 * H]
        small = lambda k: [int(v) for v in rng.integers(1, 3 * H + 1, k)]
        sizes += small(2) + [int(rng.integers(60, 62)) * H - 5] + small(2) + [int(rng.integers(60, 62)) * H + 3] + small(2 * F)
        out, total = [], 0
        for s in sizes:                                                      # cut off where the recording ends
            take = min(s, T - total)
            if take > 0:
                out.append(take)
                total += take
        return out
    if name == "sub-hop":
        # runs of 1- and 7-sample pushes that complete no frame, between ordinary ones
        sizes = [N]
        while sum(sizes) + 3 * H <= T:
            sizes += [1, 1, 1, 7, 7, 3 * H - 17]
        sizes += [H] * ((T - sum(sizes)) // H)
        assert sum(sizes) == T
        return sizes
    raise KeyError(name)


def _open(vb, pkg, rec, shape, form, max_block, channel=None):
    audio, code, channels, ch, _, _ = rec
    ext, track = ah._form(pkg, form)
    return vb.session(ah._params(pkg), ext, track, format=code, channels=channels, channel=ch if channel is None else channel,
                      frame_len=shape[0], stride=shape[1], max_block=max_block)


def _check(vb, pkg, base, fmt, shape, form, schedule):
    rec = _recording(base, fmt, *shape)
    want = _resident(vb, pkg, base, fmt, shape, form)
    sizes = _schedule(schedule, *shape)
    o = Outputs(vb, pkg, form)
    with _open(vb, pkg, rec, shape, form, max(sizes)) as sess:
        end = _feed(sess, o, rec[0], rec[1], sizes)
        assert end == (F - 1) * shape[1] + shape[0] and sess.info()[1] == F
        _assert_session(f"{fmt} {shape} {form} {schedule}", vb, pkg, o, want, shape, form)
    o.free()


# ---- 1. any split equals the resident call ---------------------------------------------------------------------------------------

def test_the_ragged_schedule_is_what_it_claims():
    for (N, H), seed in [(s, 7) for s in (NATIVE, WIDENED, (512, 512), (400, 1000))] + [(NATIVE, 11), (NATIVE, 12)]:
        sizes = _schedule("ragged", N, H, seed)
        assert sum(sizes) == (F - 1) * H + N and sizes[0] > 64 * H + N - 1 and min(sizes) >= 1
        assert sum(1 for s in sizes if 59 * H <= s <= 71 * H) >= 3
    sub = _schedule("sub-hop", *NATIVE)
    assert sub.count(1) > 100 and sub.count(7) > 100


@pytest.mark.parametrize("form", ah.FORMS)
@pytest.mark.parametrize("fmt", ah.FORMATS)
def test_every_format_and_form_ragged(vb, pkg, base, fmt, form):
    _check(vb, pkg, base, fmt, NATIVE, form, "ragged")


@pytest.mark.parametrize("schedule", ["one", "hop", "sub-hop"])
@pytest.mark.parametrize("form", ["plain", "tracked_ext"])
@pytest.mark.parametrize("fmt", ["pcm16", "f32"])
def test_the_other_schedules(vb, pkg, base, fmt, form, schedule):
    _check(vb, pkg, base, fmt, NATIVE, form, schedule)


@pytest.mark.parametrize("form", ["plain", "tracked_ext"])
@pytest.mark.parametrize("fmt", ["pcm16", "f32", "f64"])
def test_the_widened_shape_ragged(vb, pkg, base, fmt, form):
    _check(vb, pkg, base, fmt, WIDENED, form, "ragged")


@pytest.mark.parametrize("shape", [(512, 512), (400, 1000)], ids=["512/512", "400/1000"])
def test_other_shapes(vb, pkg, base, shape):
    _check(vb, pkg, base, "f64", shape, "plain", "ragged")


def test_the_returning_form_of_push(vb, pkg, base):
    """push() without out=: what analyze_frames_ex returns for the new frames, concatenated"""
    rec = _recording(base, "pcm16", *NATIVE)
    for form in ("plain", "tracked_ext"):
        want = _resident(vb, pkg, base, "pcm16", NATIVE, form)
        width = ah._width(vb, pkg, form)
        c0 = 2 if "tracked" in form else 0
        sizes = [5, 1300, 480 * 70, 7, 480 * 60]
        sizes.append((F - 1) * 480 + 1200 - sum(sizes))
        parts, pos = [], 0
        with _open(vb, pkg, rec, NATIVE, form, max(sizes)) as sess:
            for n in sizes:
                parts.append(sess.push(_block(rec[0], rec[1], pos, pos + n)))
                pos += n
        assert parts[0][0].shape[0] == 0 and parts[3][0].shape[0] == 0
        got = [np.concatenate([p[k] for p in parts], axis=1 if k == 1 else 0) for k in range(len(parts[0]))]
        assert np.array_equal(_u64(got[0][:, c0:width]), _u64(want[0][:, c0:width])) and np.array_equal(got[1], want[1])
        if c0:
            assert np.all(np.isnan(got[0][:, :2])) and np.array_equal(got[3], want[3]) and np.array_equal(_u64(got[4]), _u64(want[4]))


# ---- 2. utterance marks ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["plain", "tracked_ext"])
def test_marks(vb, pkg, base, form):
    """pushes end exactly where the frame count reaches 70, 80 and 150, and the marks are there; a further cut at frame 110 lies 30
    frames into its utterance and one at 160 lies 10 frames into its: warm = 30 and 10"""
    N, H = NATIVE
    seg = [0, 70, 80, 150]
    rec = _recording(base, "pcm16", N, H)
    want = _resident(vb, pkg, base, "pcm16", NATIVE, form, seg)
    sizes = [N + 69 * H, 10 * H, 30 * H, 40 * H, 10 * H, 40 * H]
    assert pkg.session_plan(N + 149 * H + 10 * H, 150, 40 * H, N, H).warm == 10
    o = Outputs(vb, pkg, form)
    with _open(vb, pkg, rec, NATIVE, form, max(sizes)) as sess:
        _feed(sess, o, rec[0], rec[1], sizes, marks=(70, 80, 150))
        _assert_session(f"marks {form}", vb, pkg, o, want, NATIVE, form, seg)
    o.free()


# ---- 3. bad frames across a cut --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_bad_frames_across_a_cut(vb, pkg, base, fmt):
    """NaN samples cover the frames on both sides of a block boundary: the status rows are equal, and the formant rows -- the state
    passed through -- are equal.  (At this shape the resident call reports these frames with status 0 in all three rows and NaN
    values; what is held is that the session reports and carries exactly what it does.)"""
    N, H = NATIVE
    audio, code, channels, ch, chan, which = _recording(base, fmt, N, H)
    bad = audio.copy()
    bad[95 * H:104 * H + N] = np.nan                                        # frames 93 .. 106 hold a NaN; the cut is at frame 100
    want = _reference(vb, pkg, bad, which, NATIVE, "plain")
    clean = _resident(vb, pkg, base, fmt, NATIVE, "plain")
    assert np.any(_u64(want[0][93:107]) != _u64(clean[0][93:107]), axis=1).all()      # (the NaNs reach every such frame, on both sides of the cut)
    sizes = [N + 99 * H, 30 * H, 70 * H]
    o = Outputs(vb, pkg, "plain")
    p = ah._params(pkg)
    with _open(vb, pkg, (bad, code, channels, ch, None, None), NATIVE, "plain", max(sizes)) as sess:
        _feed(sess, o, bad, code, sizes)
        got = o.download()
    o.free()
    assert np.array_equal(got[1], want[1]), ("status3", np.argwhere(got[1] != want[1])[:8])
    fa, fb = _u64(got[0][:, 2:2 + 2 * p.n_est]), _u64(want[0][:, 2:2 + 2 * p.n_est])
    assert np.array_equal(fa, fb), ("formant rows", tuple(np.argwhere(fa != fb)[0]))


# ---- 4. push_device --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["pcm16_stereo1", "pcm24", "f64"])
def test_push_device_equals_push(vb, pkg, base, fmt):
    form = "tracked_ext"
    rec = _recording(base, fmt, *NATIVE)
    audio, code = rec[0], rec[1]
    want = _resident(vb, pkg, base, fmt, NATIVE, form)
    sizes = _schedule("ragged", *NATIVE)
    dev = vb.to_device(audio.reshape(-1).view(np.uint8), np.uint8)
    sf = rec[2] * SRC_BYTES[code]
    o = Outputs(vb, pkg, form)

    def pusher(sess, pos, n, kw):
        assert sess.push_device(dev.ptr + pos * sf, n, **kw) is None
    with _open(vb, pkg, rec, NATIVE, form, max(sizes)) as sess:
        _feed(sess, o, audio, code, sizes, pusher=pusher)
        _assert_session(f"push_device {fmt}", vb, pkg, o, want, NATIVE, form)
    o.free()
    dev.free()


def test_push_device_behind_a_late_producer(pkg, base):
    """The block is produced by a copy queued on the context's stream right before the push, with no host wait (tests/stream_harness.py):
    the push reads it in stream order."""
    N, H = NATIVE
    n_fr = 60
    T = (n_fr - 1) * H + N
    hip = sh.Hip(pkg)
    stream = hip.stream_create()
    c = pkg.VoxBox(0, stream)
    try:
        _, _, _, _, chan, _ = _recording(base, "pcm16", N, H)
        host = np.ascontiguousarray(chan[:T])
        ext, track = ah._form(pkg, "ext")
        p = ah._params(pkg)
        width = int(c.L.vbx_record_doubles_ex(C.byref(p), C.byref(ext)))
        ld = width + (width & 1)
        want = c.analyze_frames_ex_pcm16(host, p, ext, None, frame_len=N, stride=H, n_frames=n_fr)
        x = c.empty(T, np.int16)
        rec, st = c.empty((n_fr, ld)), c.empty((3, n_fr), np.int32)
        sess = c.session(p, ext, None, format=1, frame_len=N, stride=H, max_block=T)

        def call():
            sess.reset()
            assert sess.push_device(x, T, out=rec, status=st, record_ld=ld) is None
        r = sh.late_producer(c, stream, call, [(x, host)], [rec, st], sh.Delay(c, pkg), hip=hip)
        assert np.array_equal(_u64(r["ref"][0][:, :width]), _u64(want[0][:, :width])) and np.array_equal(r["ref"][1], want[1])
        assert r["streams"].get("session_ingest_pcm16") == 0 and r["streams"].get("session_deliver") == 0, r["streams"]
        sess.close()
    finally:
        c.sync()
        c.close()
        hip.stream_sync(stream)
        hip.stream_destroy(stream)


# ---- 5. the session among other work ---------------------------------------------------------------------------------------------

def test_foreign_calls_between_pushes(vb, pkg, base):
    """a vbx_analyze_host call and a resident vbx_analyze_frames_f64 of another shape (more frames than any push: the context's
    workspaces grow under the session) run on the same context between pushes"""
    form = "tracked_ext"
    rec = _recording(base, "pcm16", *NATIVE)
    want = _resident(vb, pkg, base, "pcm16", NATIVE, form)
    other = np.ascontiguousarray(base[:399 * 256 + 512] * 0.5)
    sizes = _schedule("ragged", *NATIVE)
    ext, track = ah._form(pkg, form)

    def between(i):
        if i % 4 == 1:
            vb.analyze_host(other, ah._params(pkg), ext, track, chunk_frames=64, frame_len=1024, stride=512)
        if i % 4 == 3:
            vb.analyze_frames(other, ah._params(pkg), frame_len=512, stride=256)
    o = Outputs(vb, pkg, form)
    with _open(vb, pkg, rec, NATIVE, form, max(sizes)) as sess:
        _feed(sess, o, rec[0], rec[1], sizes, between=between)
        _assert_session("foreign calls between pushes", vb, pkg, o, want, NATIVE, form)
        # after a push the context holds no state for a stitch
        assert vb.L.vbx_track_stitch_f64(vb.ctx, o.rec.ptr + 16, F, o.ld, 1, F, o.rec.ptr + 16, None) == E_INVALID
    o.free()


def test_two_sessions_on_one_context(vb, pkg, base):
    """the two channels of one stereo PCM16 recording, pushes alternating, different schedules: each equals its channel's resident call"""
    form = "tracked_ext"
    N, H = NATIVE
    audio, code, channels, _, s1, which = _recording(base, "pcm16_stereo1", N, H)
    s0 = np.ascontiguousarray(audio[:, 0])
    wants = [_reference(vb, pkg, s0, which, NATIVE, form, key=("stereo0", NATIVE, form)), _resident(vb, pkg, base, "pcm16_stereo1", NATIVE, form)]
    scheds = [_schedule("ragged", N, H, seed=11), _schedule("ragged", N, H, seed=12)]
    assert scheds[0] != scheds[1]
    outs = [Outputs(vb, pkg, form), Outputs(vb, pkg, form)]
    rec = (audio, code, channels, 0, None, None)
    sessions = [_open(vb, pkg, rec, NATIVE, form, max(scheds[k]), channel=k) for k in range(2)]
    pos, nxt = [0, 0], [0, 0]
    while nxt[0] < len(scheds[0]) or nxt[1] < len(scheds[1]):
        for k in range(2):
            if nxt[k] < len(scheds[k]):
                n = scheds[k][nxt[k]]
                lo = sessions[k].info()[1]
                sessions[k].push(audio[pos[k]:pos[k] + n], **outs[k].at(lo))
                pos[k] += n
                nxt[k] += 1
    for k in range(2):
        _assert_session(f"two sessions, channel {k}", vb, pkg, outs[k], wants[k], NATIVE, form)
        sessions[k].close()
        outs[k].free()


def test_reset(vb, pkg, base):
    form = "tracked_ext"
    rec = _recording(base, "f32", *NATIVE)
    want = _resident(vb, pkg, base, "f32", NATIVE, form)
    sizes = _schedule("ragged", *NATIVE)
    junk = Outputs(vb, pkg, form)
    o = Outputs(vb, pkg, form)
    with _open(vb, pkg, rec, NATIVE, form, max(sizes)) as sess:
        _feed(sess, junk, rec[0], rec[1], sizes[:5], start=12_345)           # another stretch of the stream, a mark, a dangling tail
        sess.mark_utterance()
        sess.push(_block(rec[0], rec[1], 0, 333), **junk.at(sess.info()[1]))
        sess.reset()
        assert sess.info() == (0, 0, 0)
        _feed(sess, o, rec[0], rec[1], sizes)
        _assert_session("after a reset", vb, pkg, o, want, NATIVE, form)
    junk.free()
    o.free()


def test_pinned_and_pageable_blocks(vb, pkg, base):
    form = "tracked_ext"
    rec = _recording(base, "pcm16_stereo1", *NATIVE)
    want = _resident(vb, pkg, base, "pcm16_stereo1", NATIVE, form)
    sizes = _schedule("ragged", *NATIVE)
    pinned = vb.malloc_host(rec[0].shape, rec[0].dtype)
    pinned[...] = rec[0]
    for label, audio in (("pinned", pinned), ("pageable", rec[0])):
        o = Outputs(vb, pkg, form)
        with _open(vb, pkg, rec, NATIVE, form, max(sizes)) as sess:
            _feed(sess, o, audio, rec[1], sizes)
            _assert_session(label, vb, pkg, o, want, NATIVE, form)
        o.free()
    vb.sync()
    vb.free_host(pinned)


def test_the_block_may_be_overwritten_when_the_push_returns(vb, pkg, base):
    """the push returns when the last byte of h_block has been read: one pinned staging buffer, refilled for every push with no wait"""
    form = "plain"
    rec = _recording(base, "pcm16", *NATIVE)
    want = _resident(vb, pkg, base, "pcm16", NATIVE, form)
    sizes = _schedule("hop", *NATIVE)
    stage = vb.malloc_host(max(sizes), np.int16)
    o = Outputs(vb, pkg, form)

    def pusher(sess, pos, n, kw):
        stage[:n] = rec[0][pos:pos + n]
        assert sess.push(stage[:n], **kw) is None
        stage[:n] = -12345
    with _open(vb, pkg, rec, NATIVE, form, max(sizes)) as sess:
        _feed(sess, o, rec[0], rec[1], sizes, pusher=pusher)
        _assert_session("staging buffer reused at once", vb, pkg, o, want, NATIVE, form)
    o.free()
    vb.sync()
    vb.free_host(stage)


def test_lpc_policy_reference(vb, pkg, base, request):
    old = vb.lpc_policy
    request.addfinalizer(lambda: setattr(vb, "lpc_policy", old))
    vb.lpc_policy = pkg.LPC_POLICY_REFERENCE
    rec = _recording(base, "pcm16", *NATIVE)
    want = _resident(vb, pkg, base, "pcm16", NATIVE, "plain", policy="REFERENCE")
    plain = _REF.get(("pcm16", NATIVE, "plain", None, "EXACT"))
    assert plain is None or not np.array_equal(_u64(plain[0]), _u64(want[0]))     # (the policy matters on this recording)
    sizes = _schedule("ragged", *NATIVE)
    o = Outputs(vb, pkg, "plain")
    with _open(vb, pkg, rec, NATIVE, "plain", max(sizes)) as sess:
        _feed(sess, o, rec[0], rec[1], sizes)
        _assert_session("LPC_POLICY_REFERENCE", vb, pkg, o, want, NATIVE, "plain")
    o.free()


# ---- 6. layouts and rejections ---------------------------------------------------------------------------------------------------

def test_zero_frame_pushes_write_nothing(vb, pkg, base):
    form = "tracked_ext"
    rec = _recording(base, "pcm16", *NATIVE)
    width = ah._width(vb, pkg, form)
    ld = width + (width & 1)
    ar = la.Arena(la.DeviceBackend(vb), "zero-frame pushes")
    ar.output("records", np.float64, 4, ld)
    ar.output("status3", np.int32, 3, 4)
    ar.output("cand", np.float64, 4, 2 * KMAX)
    ar.output("count", np.int32, 1, 4)
    ar.output("peak", np.float64, 1, 4)
    ar.place()
    outs = pkg.PitchTrackOutputs(ar["cand"], ar["count"], ar["peak"], None)
    n_got = C.c_size_t(99)
    with _open(vb, pkg, rec, NATIVE, form, 2000) as sess:
        pos = 0
        for n in (1, 7, 600, 0, 591):                                       # 1199 samples: one short of the first frame
            blk = _block(rec[0], rec[1], pos, pos + n)
            vb._check(vb.L.vbx_session_push(sess.handle, blk.ctypes.data if n else None, n, ar["records"], ld, ar["status3"], 4, C.byref(outs),
                                            C.byref(n_got)))
            assert n_got.value == 0
            pos += n
        assert sess.info() == (1199, 0, 1199)
        vb._check(vb.L.vbx_session_push(sess.handle, None, 0, None, 0, None, 0, None, None))      # n_sample_frames == 0: a no-op
        vb.sync()
        out = ar.finish()
        for name, arr in out.items():
            assert la.unwritten(arr).shape[0] == arr.size, name
        # ... and the samples were carried: the next sample completes frame 0
        got = sess.push(_block(rec[0], rec[1], 1199, 1200))
        want = _resident(vb, pkg, base, "pcm16", NATIVE, form)
        assert got[0].shape[0] == 1 and np.array_equal(_u64(got[0][0, 2:width]), _u64(want[0][0, 2:width])) and np.array_equal(got[1][:, 0], want[1][:, 0])


def test_pushed_rows_fenced(vb, pkg, base):
    """padded record rows, a status leading dimension of its own, the lists the caller's: nothing outside the rows is written"""
    form = "tracked_ext"
    rec = _recording(base, "pcm32_3ch2", *NATIVE)
    want = _resident(vb, pkg, base, "pcm32_3ch2", NATIVE, form)
    width = ah._width(vb, pkg, form)
    ld = width + (width & 1) + 6
    n0 = 70
    ar = la.Arena(la.DeviceBackend(vb), "session push fenced")
    ar.output("records", np.float64, n0, width - 2, ld=ld, residue=0)
    ar.output("status3", np.int32, 3, n0, ld=n0 + 5)
    ar.output("cand", np.float64, n0, 2 * KMAX)
    ar.output("count", np.int32, 1, n0)
    ar.output("peak", np.float64, 1, n0)
    ar.place()
    outs = pkg.PitchTrackOutputs(ar["cand"], ar["count"], ar["peak"], None)
    with _open(vb, pkg, rec, NATIVE, form, 1200 + 69 * 480) as sess:
        n_got = C.c_size_t()
        blk = _block(rec[0], rec[1], 0, 1200 + 69 * 480)
        # (the arena's record rows begin at column 2, the first a tracked push writes: columns 0-1 are fence or padding)
        vb._check(vb.L.vbx_session_push(sess.handle, blk.ctypes.data, 1200 + 69 * 480, ar["records"] - 16, ld, ar["status3"], n0 + 5, C.byref(outs),
                                        C.byref(n_got)))
        assert n_got.value == n0
        out = ar.finish()
    la.assert_same_bits(ar.label, "records", out["records"], want[0][:n0, 2:width])
    la.assert_same_bits(ar.label, "status3", out["status3"], want[1][:, :n0])
    la.assert_same_bits(ar.label, "count", out["count"][0], want[3][:n0])
    la.assert_same_bits(ar.label, "peak", out["peak"][0], want[4][:n0])


def test_open_rejections(vb, pkg):
    L = vb.L
    p = ah._params(pkg)
    ext, track = ah._form(pkg, "tracked_ext")
    h = C.c_void_p()

    def fmt(format=1, channels=1, channel=0, reserved=0, chunk=0):
        f = pkg.HostAudio.make(format, channels, channel, chunk)
        f.reserved = reserved
        return f

    def opn(ctx=vb.ctx, hf=None, no_fmt=False, N=1200, H=480, prm=p, e=ext, t=track, mb=4800, out=h, no_params=False):
        hf = fmt() if hf is None else hf
        rc = L.vbx_session_open(ctx, None if no_fmt else C.byref(hf), N, H, None if no_params else C.byref(prm), None if e is None else C.byref(e),
                                None if t is None else C.byref(t), mb, None if out is None else C.byref(out))
        assert rc != 0 and not h.value, "a rejected open must not hand out a session"
        return rc
    assert opn(ctx=None) == E_INVALID and opn(no_fmt=True) == E_INVALID and opn(no_params=True) == E_INVALID and opn(out=None) == E_INVALID
    for bad in (fmt(format=0), fmt(format=6), fmt(channels=0), fmt(channels=2, channel=2), fmt(channel=-1), fmt(reserved=1), fmt(chunk=64)):
        assert opn(hf=bad) == E_INVALID, (bad.format, bad.channels, bad.channel, bad.reserved, bad.chunk_frames)
    assert opn(mb=0) == E_INVALID and opn(N=0) == E_INVALID and opn(H=0) == E_INVALID
    # what the resident call rejects from its arguments, and what only the frame loop's parts know (the warm-up call)
    assert opn(e=pkg.AnalysisExt.make(-1.0)) == E_INVALID
    assert opn(t=pkg.PitchTrackParams.make(kmax=0)) == E_INVALID and opn(t=pkg.PitchTrackParams.make(kmax=64)) == E_INVALID
    assert opn(prm=ah._params(pkg, mfcc=(65, 100.0, 8000.0))) == E_INVALID
    assert opn(prm=ah._params(pkg, mfcc=(65, 100.0, 8000.0)), e=None, t=None) == E_INVALID
    assert opn(prm=ah._params(pkg, formant_order=63)) == E_INVALID
    bad_n = ah._params(pkg)
    bad_n.n_est = 7
    assert opn(prm=bad_n) == E_INVALID
    # the context is usable afterwards
    with vb.session(p, ext, track, frame_len=1200, stride=480, max_block=4800) as sess:
        assert sess.info() == (0, 0, 0)


def test_push_rejections_leave_the_session_usable(vb, pkg, base):
    """every rejection mid-stream, nothing written, and the same session's next pushes are still bit-exact"""
    form = "tracked_ext"
    N, H = NATIVE
    rec = _recording(base, "pcm16", N, H)
    audio = rec[0]
    want = _resident(vb, pkg, base, "pcm16", NATIVE, form)
    width = ah._width(vb, pkg, form)
    ld = width + (width & 1)
    half = N + 99 * H
    rest = (F - 1) * H + N - half
    o = Outputs(vb, pkg, form)
    L = vb.L
    ar = la.Arena(la.DeviceBackend(vb), "push rejections")
    ar.output("records", np.float64, 8, ld)
    ar.output("status3", np.int32, 3, 8)
    ar.output("cand", np.float64, 8, 2 * KMAX)
    ar.output("count", np.int32, 1, 8)
    ar.output("peak", np.float64, 1, 8)
    ar.output("index", np.int32, 1, 8)
    ar.place()
    with _open(vb, pkg, rec, NATIVE, form, max(half, rest)) as sess:
        _feed(sess, o, audio, rec[1], [half])
        blk = audio[half:half + 4 * H]                                      # four frames

        def push(s=sess.handle, block=blk.ctypes.data, n=4 * H, records=ar["records"], rld=ld, st=ar["status3"], sld=8,
                 outs=(ar["cand"], ar["count"], ar["peak"], None), fn=L.vbx_session_push):
            po = None if outs is None else pkg.PitchTrackOutputs(*outs)
            return fn(s, block, n, records, rld, st, sld, None if po is None else C.byref(po), None)
        assert push(s=None) == E_INVALID and push(s=None, fn=L.vbx_session_push_device) == E_INVALID
        assert push(block=None) == E_INVALID
        assert push(n=max(half, rest) + 1) == E_INVALID                     # larger than max_block_sample_frames
        assert push(records=None) == E_INVALID
        assert push(records=ar["records"] + 8) == E_INVALID                 # misaligned
        assert push(rld=ld + 1) == E_INVALID and push(rld=width - 2) == E_INVALID
        assert push(sld=3) == E_INVALID                                     # status_ld < n
        assert push(outs=None) == E_INVALID
        assert push(outs=(None, ar["count"], ar["peak"], None)) == E_INVALID
        assert push(outs=(ar["cand"], None, ar["peak"], None)) == E_INVALID
        assert push(outs=(ar["cand"], ar["count"], None, None)) == E_INVALID          # silence_threshold != 0 needs the peaks
        assert push(outs=(ar["cand"], ar["count"], ar["peak"], ar["index"])) == E_INVALID
        dev = vb.to_device(np.zeros(64, np.int16))
        assert push(block=dev.ptr + 1, n=8, fn=L.vbx_session_push_device) == E_INVALID         # an int16 block at an odd address
        assert sess.info()[:2] == (half, 100)
        out = ar.finish()
        for name, arr in out.items():
            assert la.unwritten(arr).shape[0] == arr.size, name
        dev.free()
        _feed(sess, o, audio, rec[1], [rest], start=half)
        assert sess.info()[1] == F
        _assert_session("after the rejections", vb, pkg, o, want, NATIVE, form)
    o.free()
