"""A multi-channel live session (vbx_session_open_channels / vbx_session_push_channels) on a real MI355X.  The recording is that of
tests/test_gpu_session.py (F = 200 frames: past the point where the warm-up saturates at 64) spread over five channels of DIFFERENT
content (scaled, shifted and reversed mixes: a plane mix-up cannot pass); the default selection is channels [4, 0, 2].  The yardsticks
are the one-channel session (vbx_session_open / vbx_session_push) on each selected channel, pushed the same blocks, and the RESIDENT
call on the unpacked channel -- never the multi-channel code.  Nothing is compared with a tolerance: records, status rows, candidate
lists, counts and peaks are compared on integer views.  Both sessions write a push's rows at their global offsets into canary-filled
arrays, so equal arrays mean equal rows push by push.  References are computed once per key."""
import ctypes as C

import numpy as np
import pytest

import layout_arena as la
import stream_harness as sh
import test_gpu_analyze_host as ah
import test_gpu_session as gs
from test_gpu_session import base  # noqa: F401  (the module-scoped recording fixture)

pytestmark = pytest.mark.gpu

F = gs.F
NATIVE, WIDENED = gs.NATIVE, gs.WIDENED
KMAX = gs.KMAX
E_INVALID = -1
FORMATS = ["pcm16", "pcm24", "pcm32", "f32", "f64"]
CODE = {"pcm16": 1, "pcm24": 2, "pcm32": 3, "f32": 4, "f64": 5}
SRC_BYTES = gs.SRC_BYTES
SEL = [4, 0, 2]
_u64 = gs._u64

_REC, _ONE, _RES = {}, {}, {}


def _mix(base, channels, T):
    """[T, channels] doubles in (-1, 1): every channel its own content"""
    x = base[:T] * 0.9
    other = np.roll(x, 777)[::-1].copy()
    cols = [x, other]
    for j in range(1, channels):
        cols.append((0.55 - 0.004 * j) * np.roll(x, 313 * j) + (0.2 + 0.003 * j) * np.roll(other, 1009 * j))
    return np.stack(cols[:channels], axis=1)


def _recording(base, fmt, channels, shape, frames=F):
    """(host audio as the pushes take it, [T, channels] typed samples the resident call of a channel is given, which resident call)"""
    key = (fmt, channels, shape, frames)
    if key not in _REC:
        N, H = shape
        y = _mix(base, channels, (frames - 1) * H + N)
        if fmt == "pcm16":
            a = np.ascontiguousarray(np.round(y * 32767.0).astype(np.int16))
            _REC[key] = (a, a, "pcm16")
        elif fmt == "pcm24":
            v = np.round(y * 8388607.0).astype(np.int32)
            _REC[key] = (ah._pack24(v.reshape(-1)), v.astype(np.float64) / np.float64(8388607.0), "f64")
        elif fmt == "pcm32":
            a = np.ascontiguousarray(np.round(y * 2147483647.0).astype(np.int64).astype(np.int32))
            _REC[key] = (a, a.astype(np.float64) / np.float64(2147483647.0), "f64")
        elif fmt == "f32":
            a = np.ascontiguousarray(y.astype(np.float32))
            _REC[key] = (a, a, "f32in")
        else:
            a = np.ascontiguousarray(y)
            _REC[key] = (a, a, "f64")
    return _REC[key]


def _block(audio, fmt, channels, a, b):
    """sample frames [a, b) of the host audio"""
    return audio[3 * channels * a:3 * channels * b] if fmt == "pcm24" else audio[a:b]


def _resident(vb, pkg, typed, which, c, shape, form, seg, key):
    """the resident call on channel c of the typed samples: (records, status3[, cand, count, peak, index])"""
    key = key + (c, shape, form, None if seg is None else tuple(seg))
    if key not in _RES:
        _RES[key] = gs._reference(vb, pkg, np.ascontiguousarray(typed[:, c]), which, shape, form, seg)
    return _RES[key]


def _at_all(outs, lo):
    """the per-channel arguments of a multi-channel push whose first frame is lo"""
    at = [o.at(lo) for o in outs]
    return dict(out=[a["out"] for a in at], status=[a["status"] for a in at],
                outputs=None if at[0]["outputs"] is None else [a["outputs"] for a in at], record_ld=at[0]["record_ld"], status_ld=at[0]["status_ld"])


def _feed(sess, outs, audio, fmt, channels, sizes, marks=(), start=0, between=None, pusher=None):
    """gs._feed for either kind of session: `outs` is one Outputs (a one-channel session) or a list of them (a multi-channel one)"""
    multi = isinstance(outs, list)
    pos, c0 = start, sess.info()[0]
    for i, n in enumerate(sizes):
        lo = sess.info()[1]
        if lo in marks:
            sess.mark_utterance()
        want_n = sess.frames_of(n)
        kw = _at_all(outs, lo) if multi else outs.at(lo)
        if pusher is None:
            assert sess.push(_block(audio, fmt, channels, pos, pos + n), **kw) is None
        else:
            pusher(sess, pos, n, kw)
        pos += n
        assert sess.info()[:2] == (c0 + pos - start, lo + want_n)
        if between is not None:
            between(i)
    return pos


def _open_multi(vb, pkg, fmt, channels, sel, shape, form, max_block):
    ext, track = ah._form(pkg, form)
    return vb.session_channels(ah._params(pkg), ext, track, format=CODE[fmt], channels=channels, select=sel, frame_len=shape[0], stride=shape[1],
                               max_block=max_block)


def _open_one(vb, pkg, fmt, channels, c, shape, form, max_block):
    ext, track = ah._form(pkg, form)
    return vb.session(ah._params(pkg), ext, track, format=CODE[fmt], channels=channels, channel=c, frame_len=shape[0], stride=shape[1],
                      max_block=max_block)


def _one_channel(vb, pkg, audio, fmt, channels, c, shape, form, sizes, marks, key, frames=F):
    """what the one-channel session on channel c delivers for the same pushes (downloaded arrays), once per key"""
    key = key + (c, shape, form, tuple(sizes), tuple(marks))
    if key not in _ONE:
        o = gs.Outputs(vb, pkg, form, frames)
        with _open_one(vb, pkg, fmt, channels, c, shape, form, max(sizes)) as sess:
            _feed(sess, o, audio, fmt, channels, sizes, marks)
        _ONE[key] = o.download()
        o.free()
    return _ONE[key]


def _same(label, got, want):
    """two downloads of Outputs, bit for bit -- the canaries of rows and columns nobody wrote included"""
    assert len(got) == len(want), label
    for k, (a, b) in enumerate(zip(got, want)):
        ua, ub = (a, b) if a.dtype.kind == "i" else (_u64(a), _u64(b))
        assert ua.shape == ub.shape and np.array_equal(ua, ub), (label, "array", k, "first difference at", tuple(np.argwhere(ua != ub)[0]), int((ua != ub).sum()))


def _check(vb, pkg, base, fmt, shape, form, schedule, channels=5, sel=SEL, marks=(), seg=None, resident=True, sizes=None, audio=None,
           pusher=None, between=None, key=None):
    a0, typed, which = _recording(base, fmt, channels, shape)
    audio_in = a0 if audio is None else audio
    sizes = gs._schedule(schedule, *shape) if sizes is None else sizes
    key = (fmt, channels) if key is None else key
    outs = [gs.Outputs(vb, pkg, form) for _ in sel]
    with _open_multi(vb, pkg, fmt, channels, sel, shape, form, max(sizes)) as sess:
        end = _feed(sess, outs, audio_in, fmt, channels, sizes, marks, pusher=pusher, between=between)
        assert end == (F - 1) * shape[1] + shape[0] and sess.info()[1] == F
        for k, c in enumerate(sel):
            label = f"{fmt} x{channels} selection {sel} entry {k} (channel {c}) {shape} {form} {schedule}"
            _same(label + ": the one-channel session", outs[k].download(), _one_channel(vb, pkg, a0, fmt, channels, c, shape, form, sizes, marks, key))
            if resident:
                gs._assert_session(label + ": the resident call", vb, pkg, outs[k], _resident(vb, pkg, typed, which, c, shape, form, seg, key),
                                   shape, form, seg)
    for o in outs:
        o.free()


# ---- 1. any split, every format and form -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["plain", "tracked", "tracked_ext"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_and_form_ragged(vb, pkg, base, fmt, form):
    _check(vb, pkg, base, fmt, NATIVE, form, "ragged")


@pytest.mark.parametrize("schedule", ["one", "hop", "sub-hop"])
@pytest.mark.parametrize("fmt", ["pcm16", "f32"])
def test_the_other_schedules(vb, pkg, base, fmt, schedule):
    _check(vb, pkg, base, fmt, NATIVE, "tracked_ext", schedule)


@pytest.mark.parametrize("fmt", ["pcm16", "f32", "f64"])
def test_the_widened_shape_ragged(vb, pkg, base, fmt):
    _check(vb, pkg, base, fmt, WIDENED, "tracked_ext", "ragged")


@pytest.mark.parametrize("shape", [(512, 512), (400, 1000)], ids=["512/512", "400/1000"])
def test_other_shapes(vb, pkg, base, shape):
    _check(vb, pkg, base, "f64", shape, "plain", "ragged")


# ---- 2. utterance marks: one list for every channel ------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["plain", "tracked_ext"])
def test_marks(vb, pkg, base, form):
    """marks mid-stream at frames 70, 80 and 150 (the cuts at 110 and 160 lie 30 and 10 frames into their utterances)"""
    N, H = NATIVE
    sizes = [N + 69 * H, 10 * H, 30 * H, 40 * H, 10 * H, 40 * H]
    _check(vb, pkg, base, "pcm16", NATIVE, form, "marks", marks=(70, 80, 150), seg=[0, 70, 80, 150], sizes=sizes)


def test_two_marks_in_a_row_and_one_before_the_first_frame(vb, pkg, base):
    """mark_utterance before any frame exists (sample frames pushed, none complete) and twice between two pushes: the resident
    call's h_seg_start = [0, 90]"""
    N, H = NATIVE
    a0, typed, which = _recording(base, "f32", 5, NATIVE)
    sizes = [700, N - 700 + 89 * H, 110 * H]
    outs = [gs.Outputs(vb, pkg, "tracked_ext") for _ in SEL]
    ones = [gs.Outputs(vb, pkg, "tracked_ext") for _ in SEL]
    sessions = [(_open_multi(vb, pkg, "f32", 5, SEL, NATIVE, "tracked_ext", max(sizes)), outs)]
    sessions += [(_open_one(vb, pkg, "f32", 5, c, NATIVE, "tracked_ext", max(sizes)), ones[k]) for k, c in enumerate(SEL)]
    for sess, o in sessions:
        sess.mark_utterance()                                               # before the first sample
        _feed(sess, o, a0, "f32", 5, sizes[:1])
        sess.mark_utterance()                                               # sample frames consumed, no frame yet: still frame 0
        pos = _feed(sess, o, a0, "f32", 5, sizes[1:2], start=sizes[0])
        assert sess.info()[1] == 90
        sess.mark_utterance(); sess.mark_utterance()                        # two in a row
        _feed(sess, o, a0, "f32", 5, sizes[2:], start=pos)
        assert sess.info()[1] == F
    for k, c in enumerate(SEL):
        _same(f"marks, channel {c}: the one-channel session", outs[k].download(), ones[k].download())
        gs._assert_session(f"marks, channel {c}: the resident call", vb, pkg, outs[k],
                           _resident(vb, pkg, typed, which, c, NATIVE, "tracked_ext", [0, 90], ("f32", 5)), NATIVE, "tracked_ext", [0, 90])
    for sess, _ in sessions:
        sess.close()
    for o in outs + ones:
        o.free()


# ---- 3. one channel's NaN and Inf samples touch no other channel -----------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_channel_isolation(vb, pkg, base, fmt):
    """NaN and Inf samples in channel 0 only: a stretch that spans the block cut at frame 100, and the very last samples of the block
    that ends at frame 130 -- the end of that plane's kept region, right before the stale samples behind it.  The other channels'
    arrays are those of a clean run, bit for bit; the bad channel's are the one-channel session's."""
    N, H = NATIVE
    a0, _, _ = _recording(base, fmt, 5, NATIVE)
    bad = a0.copy()
    bad[95 * H:104 * H + N, 0] = np.nan
    bad[98 * H:99 * H, 0] = np.inf
    cut2 = N + 129 * H
    bad[cut2 - 7:cut2, 0] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf]
    sizes = [N + 99 * H, 30 * H, 70 * H]
    form = "tracked_ext"
    outs = [gs.Outputs(vb, pkg, form) for _ in SEL]
    with _open_multi(vb, pkg, fmt, 5, SEL, NATIVE, form, max(sizes)) as sess:
        _feed(sess, outs, bad, fmt, 5, sizes)
    for k, c in enumerate(SEL):
        audio = bad if c == 0 else a0
        key = (fmt, 5, "isolation") if c == 0 else (fmt, 5)
        _same(f"isolation {fmt}, channel {c}", outs[k].download(), _one_channel(vb, pkg, audio, fmt, 5, c, NATIVE, form, sizes, (), key))
    clean0 = _one_channel(vb, pkg, a0, fmt, 5, 0, NATIVE, form, sizes, (), (fmt, 5))
    assert not np.array_equal(_u64(outs[1].download()[0][93:107, 2:]), _u64(clean0[0][93:107, 2:]))       # (the bad samples do reach channel 0's rows)
    for o in outs:
        o.free()


# ---- 4. one selected channel, one channel in the stream, all 64 ------------------------------------------------------------------

def test_one_selected_channel_is_the_one_channel_session(vb, pkg, base):
    _check(vb, pkg, base, "pcm16", NATIVE, "tracked_ext", "ragged", channels=5, sel=[3])
    _check(vb, pkg, base, "pcm24", NATIVE, "plain", "ragged", channels=1, sel=[0])
    _check(vb, pkg, base, "f32", NATIVE, "tracked_ext", "ragged", channels=1, sel=[0])


def test_all_64_channels(vb, pkg, base):
    """64 of 64 channels of 16-bit PCM at 1200 / 480, 70 frames: one large block, then hop by hop"""
    N, H = NATIVE
    frames, form = 70, "tracked_ext"
    a0, typed, which = _recording(base, "pcm16", 64, NATIVE, frames)
    sizes = [N + 39 * H] + [H] * 30
    sel = list(range(64))
    outs = [gs.Outputs(vb, pkg, form, frames) for _ in sel]
    with _open_multi(vb, pkg, "pcm16", 64, sel, NATIVE, form, max(sizes)) as sess:
        _feed(sess, outs, a0, "pcm16", 64, sizes)
        assert sess.info()[1] == frames
    ext, track = ah._form(pkg, form)
    width = ah._width(vb, pkg, form)
    for c in (0, 1, 31, 62, 63):                                            # the one-channel session on a few of them ...
        _same(f"64 channels, channel {c}", outs[c].download(), _one_channel(vb, pkg, a0, "pcm16", 64, c, NATIVE, form, sizes, (), ("pcm16", 64), frames))
    for c in sel:                                                           # ... and the resident call on every one
        want = vb.analyze_frames_ex_pcm16(np.ascontiguousarray(typed[:, c]), ah._params(pkg), ext, track, frame_len=N, stride=H, n_frames=frames,
                                          lists=True)
        got = outs[c].download()
        assert np.array_equal(_u64(got[0][:, 2:width]), _u64(want[0][:, 2:width])), c
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3]) and np.array_equal(_u64(got[4]), _u64(want[4])), c
    for o in outs:
        o.free()


# ---- 5. the device form ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["pcm16", "pcm24", "f64"])
def test_push_device_equals_push(vb, pkg, base, fmt):
    a0, _, _ = _recording(base, fmt, 5, NATIVE)
    dev = vb.to_device(a0.reshape(-1).view(np.uint8), np.uint8)
    sf = 5 * SRC_BYTES[CODE[fmt]]

    def pusher(sess, pos, n, kw):
        assert sess.push_device(dev.ptr + pos * sf, n, **kw) is None
    _check(vb, pkg, base, fmt, NATIVE, "tracked_ext", "ragged", pusher=pusher, resident=False)
    dev.free()


def test_push_device_behind_a_late_producer(pkg, base):
    """The block is produced by a copy queued on the context's stream right before the push, with no host wait
    (tests/stream_harness.py): the push reads it in stream order."""
    N, H = NATIVE
    n_fr = 60
    T = (n_fr - 1) * H + N
    hip = sh.Hip(pkg)
    stream = hip.stream_create()
    c = pkg.VoxBox(0, stream)
    try:
        a0, typed, _ = _recording(base, "pcm16", 5, NATIVE)
        host = np.ascontiguousarray(a0[:T])
        ext, _ = ah._form(pkg, "ext")
        p = ah._params(pkg)
        width = int(c.L.vbx_record_doubles_ex(C.byref(p), C.byref(ext)))
        ld = width + (width & 1)
        x = c.empty((T, 5), np.int16)
        recs = [c.empty((n_fr, ld)) for _ in SEL]
        sts = [c.empty((3, n_fr), np.int32) for _ in SEL]
        sess = c.session_channels(p, ext, None, format=1, channels=5, select=SEL, frame_len=N, stride=H, max_block=T)

        def call():
            sess.reset()
            assert sess.push_device(x, T, out=recs, status=sts, record_ld=ld) is None
        r = sh.late_producer(c, stream, call, [(x, host)], recs + sts, sh.Delay(c, pkg), hip=hip)
        for k, ch in enumerate(SEL):
            want = c.analyze_frames_ex_pcm16(np.ascontiguousarray(typed[:T, ch]), p, ext, None, frame_len=N, stride=H, n_frames=n_fr)
            assert np.array_equal(_u64(r["ref"][k][:, :width]), _u64(want[0][:, :width])) and np.array_equal(r["ref"][len(SEL) + k], want[1]), ch
        assert r["streams"].get("session_ingest_all_pcm16") == 0 and r["streams"].get("session_deliver_all") == 0, r["streams"]
        sess.close()
    finally:
        c.sync()
        c.close()
        hip.stream_sync(stream)
        hip.stream_destroy(stream)


# ---- 6. the session among other work ---------------------------------------------------------------------------------------------

def test_foreign_calls_between_pushes(vb, pkg, base):
    """a vbx_analyze_host call with a segment list of its own and a resident vbx_analyze_frames_f64 of another shape run on the same
    context between pushes (the context's staged segment list and its workspaces change under the session)"""
    other = np.ascontiguousarray(base[:399 * 256 + 512] * 0.5)
    ext, track = ah._form(pkg, "tracked_ext")

    def between(i):
        if i % 4 == 1:
            vb.analyze_host(other, ah._params(pkg), ext, track, chunk_frames=64, seg_start=[0, 50, 120], frame_len=1024, stride=512)
        if i % 4 == 3:
            vb.analyze_frames(other, ah._params(pkg), frame_len=512, stride=256)
    _check(vb, pkg, base, "pcm16", NATIVE, "tracked_ext", "ragged", between=between, resident=False)


def test_a_multi_channel_and_a_one_channel_session_on_one_context(vb, pkg, base):
    """pushes alternate between a multi-channel session on channels [4, 0, 2] and a one-channel session on channel 1, on different
    schedules"""
    form = "tracked_ext"
    N, H = NATIVE
    a0, typed, which = _recording(base, "pcm16", 5, NATIVE)
    scheds = [gs._schedule("ragged", N, H, seed=11), gs._schedule("ragged", N, H, seed=12)]
    outs, one = [gs.Outputs(vb, pkg, form) for _ in SEL], gs.Outputs(vb, pkg, form)
    sessions = [_open_multi(vb, pkg, "pcm16", 5, SEL, NATIVE, form, max(scheds[0])), _open_one(vb, pkg, "pcm16", 5, 1, NATIVE, form, max(scheds[1]))]
    pos, nxt = [0, 0], [0, 0]
    while nxt[0] < len(scheds[0]) or nxt[1] < len(scheds[1]):
        for k in range(2):
            if nxt[k] < len(scheds[k]):
                n = scheds[k][nxt[k]]
                lo = sessions[k].info()[1]
                sessions[k].push(a0[pos[k]:pos[k] + n], **(_at_all(outs, lo) if k == 0 else one.at(lo)))
                pos[k] += n
                nxt[k] += 1
    for k, c in enumerate(SEL):
        gs._assert_session(f"beside a one-channel session, channel {c}", vb, pkg, outs[k],
                           _resident(vb, pkg, typed, which, c, NATIVE, form, None, ("pcm16", 5)), NATIVE, form)
    gs._assert_session("the one-channel session beside it", vb, pkg, one, _resident(vb, pkg, typed, which, 1, NATIVE, form, None, ("pcm16", 5)), NATIVE, form)
    for s in sessions:
        s.close()
    for o in outs + [one]:
        o.free()


def test_reset(vb, pkg, base):
    form = "tracked_ext"
    a0, _, _ = _recording(base, "f32", 5, NATIVE)
    sizes = gs._schedule("ragged", *NATIVE)
    junk = [gs.Outputs(vb, pkg, form) for _ in SEL]
    outs = [gs.Outputs(vb, pkg, form) for _ in SEL]
    with _open_multi(vb, pkg, "f32", 5, SEL, NATIVE, form, max(sizes)) as sess:
        _feed(sess, junk, a0, "f32", 5, sizes[:5], start=12_345)             # another stretch of the stream, a mark, a dangling tail
        sess.mark_utterance()
        sess.push(a0[:333], **_at_all(junk, sess.info()[1]))
        sess.reset()
        assert sess.info() == (0, 0, 0)
        _feed(sess, outs, a0, "f32", 5, sizes)
    for k, c in enumerate(SEL):
        _same(f"after a reset, channel {c}", outs[k].download(), _one_channel(vb, pkg, a0, "f32", 5, c, NATIVE, form, sizes, (), ("f32", 5)))
    for o in junk + outs:
        o.free()


def test_pinned_and_pageable_blocks(vb, pkg, base):
    a0, _, _ = _recording(base, "pcm16", 5, NATIVE)
    pinned = vb.malloc_host(a0.shape, a0.dtype)
    pinned[...] = a0
    for audio in (pinned, a0):
        _check(vb, pkg, base, "pcm16", NATIVE, "tracked_ext", "ragged", audio=audio, resident=False)
    # blocks above the staging limit take the copy stream: three blocks of more than 128 KiB
    sizes = [NATIVE[0] + 69 * 480, 70 * 480, 60 * 480]
    for audio in (pinned, a0):
        _check(vb, pkg, base, "pcm16", NATIVE, "tracked_ext", "three", sizes=sizes, audio=audio, resident=False)
    vb.sync()
    vb.free_host(pinned)


def test_the_block_may_be_overwritten_when_the_push_returns(vb, pkg, base):
    """the push returns when the last byte of h_block has been read: one pinned buffer, refilled for every push with no wait -- hop
    by hop (the staged route) and in three large blocks (the copy stream)"""
    a0, _, _ = _recording(base, "pcm16", 5, NATIVE)
    for name, sizes in (("hop", None), ("three", [NATIVE[0] + 69 * 480, 70 * 480, 60 * 480])):
        n_max = max(sizes) if sizes else NATIVE[0]
        stage = vb.malloc_host((n_max, 5), np.int16)

        def pusher(sess, pos, n, kw):
            stage[:n] = a0[pos:pos + n]
            assert sess.push(stage[:n], **kw) is None
            stage[:n] = -12345
        _check(vb, pkg, base, "pcm16", NATIVE, "plain", name, sizes=sizes, pusher=pusher, resident=False)
        vb.sync()
        vb.free_host(stage)


def test_lpc_policy_reference(vb, pkg, base, request):
    old = vb.lpc_policy
    request.addfinalizer(lambda: setattr(vb, "lpc_policy", old))
    vb.lpc_policy = pkg.LPC_POLICY_REFERENCE
    _check(vb, pkg, base, "pcm16", NATIVE, "plain", "ragged", key=("pcm16", 5, "REFERENCE"))
    exact = _RES.get(("pcm16", 5, 0, NATIVE, "plain", None))
    ref = _RES[("pcm16", 5, "REFERENCE", 0, NATIVE, "plain", None)]
    assert exact is None or not np.array_equal(_u64(exact[0]), _u64(ref[0]))          # (the policy matters on this recording)


# ---- 7. layouts and rejections ---------------------------------------------------------------------------------------------------

def _arena(vb, label, K, rows, ld, width, st_ld):
    ar = la.Arena(la.DeviceBackend(vb), label)
    for k in range(K):
        ar.output(f"records{k}", np.float64, rows, width - 2, ld=ld, residue=0)
        ar.output(f"status{k}", np.int32, 3, rows, ld=st_ld)
        ar.output(f"cand{k}", np.float64, rows, 2 * KMAX)
        ar.output(f"count{k}", np.int32, 1, rows)
        ar.output(f"peak{k}", np.float64, 1, rows)
    ar.place()
    return ar


def _entries(pkg, ar, K, records=None, outputs=None, status=None):
    """(the vbx_channel_outputs array, what keeps its pointers alive); the arena's record rows begin at column 2, the first a tracked
    push writes"""
    ent = (pkg.ChannelOutputs * K)()
    keep = []
    for k in range(K):
        po = pkg.PitchTrackOutputs(ar[f"cand{k}"], ar[f"count{k}"], ar[f"peak{k}"], None) if outputs is None else outputs(k)
        keep.append(po)
        ent[k].records = ar[f"records{k}"] - 16 if records is None else records(k)
        ent[k].status3 = ar[f"status{k}"] if status is None else status(k)
        ent[k].outputs = None if po is None else C.pointer(po)
    return ent, keep


def test_zero_frame_pushes_write_nothing(vb, pkg, base):
    form = "tracked_ext"
    a0, _, _ = _recording(base, "pcm16", 5, NATIVE)
    width = ah._width(vb, pkg, form)
    ld = width + (width & 1)
    ar = _arena(vb, "zero-frame pushes", 3, 4, ld, width, 4)
    ent, keep = _entries(pkg, ar, 3)
    n_got = C.c_size_t(99)
    with _open_multi(vb, pkg, "pcm16", 5, SEL, NATIVE, form, 2000) as sess:
        pos = 0
        for n in (1, 7, 600, 0, 591):                                       # 1199 sample frames: one short of the first frame
            blk = a0[pos:pos + n]
            vb._check(vb.L.vbx_session_push_channels(sess.handle, blk.ctypes.data if n else None, n, ent, ld, 4, C.byref(n_got)))
            assert n_got.value == 0
            pos += n
        assert sess.info() == (1199, 0, 1199)
        vb._check(vb.L.vbx_session_push_channels(sess.handle, None, 0, None, 0, 0, None))      # n_sample_frames == 0: a no-op
        vb.sync()
        out = ar.finish()
        for name, arr in out.items():
            assert la.unwritten(arr).shape[0] == arr.size, name
        got = sess.push(a0[1199:1200])                                      # ... and the samples were carried: the next one completes frame 0
    for k, c in enumerate(SEL):
        want = _one_channel(vb, pkg, a0, "pcm16", 5, c, NATIVE, form, [1200], (), ("pcm16", 5, "first"), 1)
        assert got[k][0].shape[0] == 1 and np.array_equal(_u64(got[k][0][0, 2:width]), _u64(want[0][0, 2:width])) and np.array_equal(got[k][1], want[1])


def test_pushed_rows_fenced(vb, pkg, base):
    """padded record rows, a status leading dimension of its own, the lists the caller's, for every channel: nothing outside the rows
    is written"""
    form = "tracked_ext"
    N, H = NATIVE
    a0, typed, which = _recording(base, "pcm32", 5, NATIVE)
    width = ah._width(vb, pkg, form)
    ld = width + (width & 1) + 6
    n0 = 70
    ar = _arena(vb, "multi-channel push fenced", 3, n0, ld, width, n0 + 5)
    ent, keep = _entries(pkg, ar, 3)
    with _open_multi(vb, pkg, "pcm32", 5, SEL, NATIVE, form, N + 69 * H) as sess:
        n_got = C.c_size_t()
        vb._check(vb.L.vbx_session_push_channels(sess.handle, a0.ctypes.data, N + 69 * H, ent, ld, n0 + 5, C.byref(n_got)))
        assert n_got.value == n0
        out = ar.finish()
    for k, c in enumerate(SEL):
        want = _resident(vb, pkg, typed, which, c, NATIVE, form, None, ("pcm32", 5))
        la.assert_same_bits(ar.label, f"records{k}", out[f"records{k}"], want[0][:n0, 2:width])
        la.assert_same_bits(ar.label, f"status{k}", out[f"status{k}"], want[1][:, :n0])
        la.assert_same_bits(ar.label, f"count{k}", out[f"count{k}"][0], want[3][:n0])
        la.assert_same_bits(ar.label, f"peak{k}", out[f"peak{k}"][0], want[4][:n0])


def test_open_rejections(vb, pkg):
    L = vb.L
    p = ah._params(pkg)
    ext, track = ah._form(pkg, "tracked_ext")
    h = C.c_void_p()
    sel3 = np.ascontiguousarray(SEL, dtype=np.int32)

    def fmt(format=1, channels=5, channel=0, reserved=0, chunk=0):
        f = pkg.HostAudio.make(format, channels, channel, chunk)
        f.reserved = reserved
        return f

    def opn(ctx=vb.ctx, hf=None, sel=sel3, n_sel=3, N=1200, H=480, prm=p, e=ext, t=track, mb=4800, out=h):
        hf = fmt() if hf is None else hf
        rc = L.vbx_session_open_channels(ctx, C.byref(hf), None if sel is None else sel.ctypes.data, n_sel, N, H, C.byref(prm),
                                         None if e is None else C.byref(e), None if t is None else C.byref(t), mb, None if out is None else C.byref(out))
        assert rc != 0 and not h.value, "a rejected open must not hand out a session"
        return rc
    assert opn(ctx=None) == E_INVALID and opn(out=None) == E_INVALID
    for bad in (fmt(format=0), fmt(format=6), fmt(channels=0), fmt(channel=1), fmt(reserved=1), fmt(chunk=64)):
        assert opn(hf=bad) == E_INVALID, (bad.format, bad.channels, bad.channel, bad.reserved, bad.chunk_frames)
    # a bad selection: none, empty, more than the channels, out of range, repeated
    assert opn(sel=None) == E_INVALID and opn(n_sel=0) == E_INVALID
    assert opn(hf=fmt(channels=2)) == E_INVALID
    for bad in ([4, 0, 5], [4, 0, -1], [4, 0, 4]):
        assert opn(sel=np.ascontiguousarray(bad, dtype=np.int32)) == E_INVALID, bad
    assert opn(hf=fmt(channels=70), sel=np.arange(65, dtype=np.int32), n_sel=65) == E_INVALID       # above VBX_HOST_MAX_CHANNELS
    assert opn(mb=0) == E_INVALID and opn(N=0) == E_INVALID and opn(H=0) == E_INVALID
    assert opn(H=1, mb=1 << 31) == E_INVALID                                 # more than 0x7fffffff frames in the largest call
    # what the resident call rejects from its arguments, and what only the frame loop's parts know (the warm-up call)
    assert opn(e=pkg.AnalysisExt.make(-1.0)) == E_INVALID
    assert opn(t=pkg.PitchTrackParams.make(kmax=0)) == E_INVALID and opn(t=pkg.PitchTrackParams.make(kmax=64)) == E_INVALID
    assert opn(prm=ah._params(pkg, mfcc=(65, 100.0, 8000.0))) == E_INVALID
    assert opn(prm=ah._params(pkg, formant_order=63)) == E_INVALID
    # the context is usable afterwards
    with vb.session_channels(p, ext, track, channels=5, select=SEL, frame_len=1200, stride=480, max_block=4800) as sess:
        assert sess.info() == (0, 0, 0)


def test_push_rejections_leave_the_session_usable(vb, pkg, base):
    """every rejection mid-stream, nothing written, and the same session's next pushes are still bit-exact; the one-channel and the
    multi-channel calls do not mix"""
    form = "tracked_ext"
    N, H = NATIVE
    a0, _, _ = _recording(base, "pcm16", 5, NATIVE)
    width = ah._width(vb, pkg, form)
    ld = width + (width & 1)
    half = N + 99 * H
    rest = (F - 1) * H + N - half
    sizes = [half, rest]
    outs = [gs.Outputs(vb, pkg, form) for _ in SEL]
    L = vb.L
    ar = _arena(vb, "multi-channel push rejections", 3, 8, ld, width, 8)
    index = vb.empty(8, np.int32)
    with _open_multi(vb, pkg, "pcm16", 5, SEL, NATIVE, form, max(sizes)) as sess, \
            _open_one(vb, pkg, "pcm16", 5, 0, NATIVE, form, max(sizes)) as single:
        _feed(sess, outs, a0, "pcm16", 5, [half])
        blk = a0[half:half + 4 * H]                                          # four frames
        good, keep = _entries(pkg, ar, 3)

        def push(s=sess.handle, block=blk.ctypes.data, n=4 * H, ent=good, rld=ld, sld=8, fn=L.vbx_session_push_channels):
            return fn(s, block, n, ent, rld, sld, None)

        def outputs_of(bad_k, make):
            return lambda k: make(k) if k == bad_k else pkg.PitchTrackOutputs(ar[f"cand{k}"], ar[f"count{k}"], ar[f"peak{k}"], None)
        assert push(s=None) == E_INVALID and push(s=None, fn=L.vbx_session_push_channels_device) == E_INVALID
        assert push(block=None) == E_INVALID
        assert push(n=max(sizes) + 1) == E_INVALID                           # larger than max_block_sample_frames
        assert push(ent=None) == E_INVALID
        assert push(ent=_entries(pkg, ar, 3, records=lambda k: None if k == 1 else ar[f"records{k}"] - 16)[0]) == E_INVALID
        assert push(ent=_entries(pkg, ar, 3, records=lambda k: ar[f"records{k}"] - 8)[0]) == E_INVALID              # misaligned
        assert push(ent=_entries(pkg, ar, 3, records=lambda k: ar[f"records{k % 2}"] - 16)[0]) == E_INVALID      # entries 0 and 2 are one array
        assert push(ent=_entries(pkg, ar, 3, records=lambda k: ar["records0"] - 16 + k * 3 * ld * 8)[0]) == E_INVALID  # [4, ld] ranges three rows apart overlap
        assert push(rld=ld + 1) == E_INVALID and push(rld=width - 2) == E_INVALID
        assert push(sld=3) == E_INVALID                                      # status_ld < n
        for bad in (lambda k: None, lambda k: pkg.PitchTrackOutputs(None, ar[f"count{k}"], ar[f"peak{k}"], None),
                    lambda k: pkg.PitchTrackOutputs(ar[f"cand{k}"], None, ar[f"peak{k}"], None),
                    lambda k: pkg.PitchTrackOutputs(ar[f"cand{k}"], ar[f"count{k}"], None, None),      # silence_threshold != 0 needs the peaks
                    lambda k: pkg.PitchTrackOutputs(ar[f"cand{k}"], ar[f"count{k}"], ar[f"peak{k}"], index.ptr)):
            ent, keep2 = _entries(pkg, ar, 3, outputs=outputs_of(2, bad))
            assert push(ent=ent) == E_INVALID
        dev = vb.to_device(np.zeros(64, np.int16))
        assert push(block=dev.ptr + 1, n=8, fn=L.vbx_session_push_channels_device) == E_INVALID        # an int16 block at an odd address
        # the calls do not mix
        po = pkg.PitchTrackOutputs(ar["cand0"], ar["count0"], ar["peak0"], None)
        for fn in (L.vbx_session_push, L.vbx_session_push_device):
            assert fn(sess.handle, blk.ctypes.data, 4 * H, ar["records0"] - 16, ld, ar["status0"], 8, C.byref(po), None) == E_INVALID
        assert L.vbx_session_path_bind(sess.handle, 1.0, 64, ar["records0"] - 16, 2, None, None, ar["records1"] - 16) == E_INVALID
        assert push(s=single.handle) == E_INVALID and push(s=single.handle, fn=L.vbx_session_push_channels_device) == E_INVALID
        assert sess.info()[:2] == (half, 100) and single.info() == (0, 0, 0)
        out = ar.finish()
        for name, arr in out.items():
            assert la.unwritten(arr).shape[0] == arr.size, name
        dev.free()
        _feed(sess, outs, a0, "pcm16", 5, [rest], start=half)
        assert sess.info()[1] == F
        for k, c in enumerate(SEL):
            _same(f"after the rejections, channel {c}", outs[k].download(),
                  _one_channel(vb, pkg, a0, "pcm16", 5, c, NATIVE, form, sizes, (), ("pcm16", 5)))
    index.free()
    for o in outs:
        o.free()


# ---- 8. the launches of a push do not depend on the number of channels ------------------------------------------------------------

def test_launches_do_not_depend_on_n_sel(vb, pkg, base):
    """one steady-state 1-hop push (1200 / 480, 16-bit PCM, every part on, warm = 64), profiled: the names and launch counts are the
    same for 1, 2 and 5 selected channels, and the ingest and the deliver run exactly once"""
    N, H = NATIVE
    form = "tracked_ext"
    a0, _, _ = _recording(base, "pcm16", 5, NATIVE)
    reports = {}
    for sel in ([3], [1, 4], [4, 0, 2, 1, 3]):
        outs = [gs.Outputs(vb, pkg, form) for _ in sel]
        with _open_multi(vb, pkg, "pcm16", 5, sel, NATIVE, form, N + 79 * H) as sess:
            pos = _feed(sess, outs, a0, "pcm16", 5, [N + 79 * H, H, H])
            assert pkg.session_plan(pos, 0, H, N, H).warm == 64
            vb.sync()
            vb.profile(True)
            vb.profile_reset()
            try:
                _feed(sess, outs, a0, "pcm16", 5, [H], start=pos)
                vb.sync()
                reports[len(sel)] = {name: cnt for name, (_, cnt) in vb.profile_report().items()}
            finally:
                vb.profile(False)
        for o in outs:
            o.free()
    assert reports[1] == reports[2] == reports[5], reports
    rep = reports[5]
    assert rep["session_ingest_all_pcm16"] == 1 and rep["session_deliver_all"] == 1 and rep["tracker_stitch_all"] == 1, rep
    assert [n for n in rep if n.startswith("session_ingest")] == ["session_ingest_all_pcm16"] and "session_deliver" not in rep, rep
    assert "pcm16" not in rep                                               # 1200-sample PCM16 frames stay on the kernels that read without a widening copy
