"""vbx_analyze_clips on a real MI355X: a batch of variable-length clips in separate device buffers from ONE call.  The yardstick is
the RESIDENT call per clip on the clip's own buffer (vbx_analyze_frames_ex_pcm16 / _f32in / _f64; for PCM24 _f64 on the correctly
rounded quotients) -- never the new code against itself -- and every comparison is on uint64 / uint32 views: records, the three
status rows, candidate lists, counts, peaks and list indices, rows [row_start_b, row_start_b + n_rows_b) of the batch against the
whole output of clip b's own call.  Each clip has its own content (its own stretch of the recording at its own gain: a mix-up of
clips cannot pass).  References are computed once per key and shared.

Shapes: 1200/480 and 1024/512 at PCM16, F32 and F64; 400/160, 4100/2050 (frames beyond 4096 samples) and 400/1000 (stride >
frame_len) at F64; PCM24 at 1200/480.  Lengths: N - 1, N, N + H/2, N + H/2 + 1, N + H, 0, N + 299 H, one clip of 400 frames (the
chunked tracker scan: 384 frames and more) beside short ones.  Forms: plain, tracked (kmax 4; silence_threshold 0 and 0.03; all four
output arrays and none), ext (ratio 0.25, RMS).  group_frames 64 (many groups), a value that puts a cut right behind a one-frame clip,
and 0 must give the same bits.  (Frames beyond 4096 samples: the long-frame kernels split a frame's sums by the call's frame
count, so the plan makes every such clip a group of its own; the test holds that shape to the same bits.)"""
import ctypes as C

import numpy as np
import pytest

import layout_arena as la
import stream_harness as sh
import test_gpu_analyze_host as ah
from test_gpu_stream_order import hip, sctx  # noqa: F401  (fixtures: a context on a caller-created stream)

pytestmark = pytest.mark.gpu

SR = 48000.0
E_INVALID = -1
CODE = {"pcm16": 1, "pcm24": 2, "pcm32": 3, "f32": 4, "f64": 5}
DTYPE = {"pcm16": np.int16, "pcm24": np.uint8, "pcm32": np.int32, "f32": np.float32, "f64": np.float64}
SHAPES = [("pcm16", 1200, 480), ("f32", 1200, 480), ("f64", 1200, 480), ("pcm24", 1200, 480),
          ("pcm16", 1024, 512), ("f32", 1024, 512), ("f64", 1024, 512),
          ("f64", 400, 160), ("f64", 4100, 2050), ("f64", 400, 1000)]
_REF = {}


def _u(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind in "iu" else a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def base(vb):
    """25 s of the synthetic speech as doubles in (-1, 1)"""
    d = vb.synth_speech(1_200_000, sample_offset=7 * 48000 + 99)
    a = d.numpy()
    d.free()
    return a


class Clip:
    """one clip: `ident` names its content; `raw` is what lies in device memory, `typed` what the resident call is given"""

    def __init__(self, base, fmt, k, length, poison=None):
        off = (k * 40_009) % (base.size - length - 1)
        y = base[off:off + length] * (0.9 - 0.013 * (k % 40))
        self.fmt, self.length, self.ident = fmt, length, (fmt, k, length, poison)
        if fmt == "pcm16":
            self.raw = self.typed = np.round(y * 32767.0).astype(np.int16)
            self.which = "pcm16"
        elif fmt == "pcm24":
            v = np.round(y * 8388607.0).astype(np.int32)
            self.raw, self.typed, self.which = ah._pack24(v), v.astype(np.float64) / np.float64(8388607.0), "f64"
        elif fmt == "pcm32":
            v = np.round(y * 2147483647.0).astype(np.int64).astype(np.int32)
            self.raw, self.typed, self.which = v, v.astype(np.float64) / np.float64(2147483647.0), "f64"
        elif fmt == "f32":
            self.raw = self.typed = y.astype(np.float32)
            self.which = "f32in"
        else:
            self.raw = self.typed = y.copy()
            self.which = "f64"
        if poison is not None and length >= 3:                                   # NaN and Inf in the clip's last samples
            self.raw[-1], self.raw[-2], self.raw[-3] = np.nan, np.inf, -np.inf


def _form(pkg, form):
    """(ext, track, lists): plain / ext / tracked (silence 0.03, all four arrays) / tracked0 (silence 0) / *_none (no arrays)"""
    ext = pkg.AnalysisExt.make(0.25, rms=True) if "ext" in form else None
    track = None
    if "tracked" in form:
        track = pkg.PitchTrackParams.make(kmax=4, silence_threshold=0.0 if "tracked0" in form else 0.03)
    return ext, track, track is not None and "none" not in form


def _width(vb, pkg, form):
    ext = _form(pkg, form)[0]
    p = ah._params(pkg)
    return int(vb.L.vbx_record_doubles_ex(C.byref(p), None if ext is None else C.byref(ext)))


def _resident(vb, pkg, clip, N, H, form, policy="EXACT"):
    """the resident call on the clip's own samples, one segment: (records, status3[, cand, count, peak, index])"""
    key = (clip.ident, N, H, form, policy)
    if key not in _REF:
        ext, track, lists = _form(pkg, form)
        fn = {"pcm16": vb.analyze_frames_ex_pcm16, "f32in": vb.analyze_frames_ex_f32in, "f64": vb.analyze_frames_ex}[clip.which]
        _REF[key] = fn(clip.typed, ah._params(pkg), ext, track, frame_len=N, stride=H, lists=lists)
    return _REF[key]


def _upload(vb, clips):
    return [vb.to_device(c.raw, DTYPE[c.fmt]) if c.length else None for c in clips]


def _batch(vb, pkg, clips, dev, N, H, form, group_frames):
    ext, track, lists = _form(pkg, form)
    ptrs = [0 if d is None else d.ptr for d in dev]
    return vb.analyze_clips(ptrs, [c.length for c in clips], ah._params(pkg), ext, track, format=CODE[clips[0].fmt], group_frames=group_frames,
                            frame_len=N, stride=H, lists=lists)


def _compare(label, vb, pkg, got, clips, N, H, form, policy="EXACT"):
    """rows [row_start_b, +n_rows_b) of every array of the batch == clip b's own resident call, bit for bit"""
    rows, total, _ = pkg.clips_plan([c.length for c in clips], N, H)
    w = _width(vb, pkg, form)
    assert got[0].shape[0] == total and got[1].shape == (3, total), (label, got[0].shape, got[1].shape, total)
    for b, c in enumerate(clips):
        r0, n = int(rows[b, 0]), int(rows[b, 1])
        if n == 0:
            continue
        want = _resident(vb, pkg, c, N, H, form, policy)
        assert want[0].shape[0] == n
        pairs = [("records", got[0][r0:r0 + n, :w], want[0][:, :w]), ("status", got[1][:, r0:r0 + n], want[1])]
        for k, name in enumerate(("cand", "count", "peak", "index"), 2):
            if len(got) > k:
                pairs.append((name, got[k][r0:r0 + n], want[k]))
        for name, g, x in pairs:
            ug, ux = _u(g), _u(x)
            assert ug.shape == ux.shape and np.array_equal(ug, ux), \
                (label, "clip", b, "length", c.length, name, "first difference at", tuple(np.argwhere(ug != ux)[0]), int((ug != ux).sum()))


def _lengths(N, H, long_clip):
    ls = [N + 70 * H + 1, N, N - 1, N + H // 2, N + H // 2 + 1, N + H, 0, N + 299 * H, N + 3 * H + 7, N + 20 * H]
    return ls + ([N + 399 * H, N + 2 * H] if long_clip else [])


def _cut_behind_the_one_frame_clip(pkg, lengths, N, H):
    """a group_frames that closes the first group right behind clip 1, which has one frame"""
    gf = -(-lengths[0] // H) + 1
    rows, _, groups = pkg.clips_plan(lengths, N, H, gf)
    nxt = next(b for b in range(2, len(lengths)) if rows[b, 1] > 0)
    assert gf >= 64 and rows[1, 1] == 1 and rows[1, 2] == 0 and rows[nxt, 2] == 1 and groups > 2
    return gf


@pytest.mark.parametrize("fmt,N,H", SHAPES, ids=[f"{f}-{n}/{h}" for f, n, h in SHAPES])
def test_every_clip_equals_its_own_resident_call(vb, pkg, base, fmt, N, H):
    lengths = _lengths(N, H, long_clip=(N, H) == (1200, 480))
    clips = [Clip(base, fmt, k, ln) for k, ln in enumerate(lengths)]
    dev = _upload(vb, clips)
    if N <= 4096:
        cut = _cut_behind_the_one_frame_clip(pkg, lengths, N, H)
        assert pkg.clips_plan(lengths, N, H, 64)[2] >= 4 and pkg.clips_plan(lengths, N, H, 0)[2] == 1
    else:                                                                         # longer frames: every clip is a group by itself
        cut = 100
        assert pkg.clips_plan(lengths, N, H, 0)[2] == sum(1 for ln in lengths if ln >= N)
    for form in ("plain", "tracked", "ext"):
        for gf in (64, cut, 0):
            got = _batch(vb, pkg, clips, dev, N, H, form, gf)
            _compare(f"{fmt} {N}/{H} {form} group_frames {gf}", vb, pkg, got, clips, N, H, form)
    for d in dev:
        if d is not None:
            d.free()


@pytest.mark.parametrize("form", ["tracked0", "tracked_none", "tracked0_none", "tracked_ext"])
def test_the_tracked_variants(vb, pkg, base, form):
    """silence_threshold 0 and 0.03, with all four output arrays and with none (the lists live in the context's workspace)"""
    N, H = 1200, 480
    lengths = _lengths(N, H, long_clip=False)
    clips = [Clip(base, "pcm16", k, ln) for k, ln in enumerate(lengths)]
    dev = _upload(vb, clips)
    for gf in (64, 0):
        got = _batch(vb, pkg, clips, dev, N, H, form, gf)
        assert len(got) == (2 if "none" in form else 6)
        _compare(f"{form} group_frames {gf}", vb, pkg, got, clips, N, H, form)
    for d in dev:
        if d is not None:
            d.free()


def test_the_reference_lpc_policy(vb, pkg, base):
    N, H = 1200, 480
    clips = [Clip(base, "f64", k, ln) for k, ln in enumerate([N + 30 * H, N, N + 5 * H + 3, N + 80 * H])]
    dev = _upload(vb, clips)
    before = vb.lpc_policy
    try:
        vb.lpc_policy = pkg.LPC_POLICY_REFERENCE
        for gf in (64, 0):
            got = _batch(vb, pkg, clips, dev, N, H, "plain", gf)
            _compare(f"REFERENCE group_frames {gf}", vb, pkg, got, clips, N, H, "plain", policy="REFERENCE")
    finally:
        vb.lpc_policy = before
    for d in dev:
        d.free()


@pytest.mark.parametrize("fmt", ["f64", "f32"])
def test_a_nan_in_one_clip_touches_no_other_clip(vb, pkg, base, fmt):
    N, H = 1200, 480
    lengths = [N + 4 * H, N + 9 * H + 1, N, N + 6 * H + 470, N + 2 * H]
    clean = [Clip(base, fmt, k, ln) for k, ln in enumerate(lengths)]
    dirty = list(clean)
    dirty[1] = Clip(base, fmt, 1, lengths[1], poison=True)                        # its last samples lie right before clip 2's first
    dev = _upload(vb, dirty)
    for form in ("tracked", "ext"):
        got = _batch(vb, pkg, dirty, dev, N, H, form, 0)
        # every other clip: the rows of a clean run; the poisoned clip: its own resident call's
        _compare(f"isolation {fmt} {form}", vb, pkg, got, dirty, N, H, form)
        a, b = _resident(vb, pkg, clean[1], N, H, form)[0], _resident(vb, pkg, dirty[1], N, H, form)[0]
        assert not np.array_equal(_u(a), _u(b)), "the poison changed nothing: the case is vacuous"
    for d in dev:
        d.free()


def test_overlapping_and_repeated_clips_and_the_padded_batch(vb, pkg, base):
    N, H = 1200, 480
    # one buffer; the clips are windows into it that overlap, repeat and nest
    whole = Clip(base, "pcm16", 3, 40_000)
    d = vb.to_device(whole.raw, np.int16)
    wins = [(0, 40_000), (0, 40_000), (100, 5_000), (101, 5_000), (2_000, 1_200), (0, 1_199), (39_000, 1_000), (7, 20_001)]
    refs = []
    for o, ln in wins:
        c = Clip(base, "pcm16", 0, ln)
        c.raw = c.typed = whole.raw[o:o + ln]
        c.ident = ("window", o, ln)
        refs.append(c)
    got = vb.analyze_clips([d.ptr + 2 * o for o, _ in wins], [ln for _, ln in wins], ah._params(pkg), None, _form(pkg, "tracked")[1],
                           format=CODE["pcm16"], group_frames=64, frame_len=N, stride=H, lists=True)
    _compare("windows into one buffer", vb, pkg, got, refs, N, H, "tracked")
    d.free()
    # the padded [B, Tmax] form: row b's first lengths[b] samples are clip b; the padding holds other rows' poison (NaN)
    for fmt, tmax in (("f32", 9_001), ("pcm16", 9_003)):
        lengths = [9_001, 1_200, 0, 4_321, 1_199, 8_000]
        clips = [Clip(base, fmt, 50 + k, ln) for k, ln in enumerate(lengths)]
        pad = np.full((len(lengths), tmax), np.nan if fmt == "f32" else -32768, DTYPE[fmt])
        for b, c in enumerate(clips):
            pad[b, :c.length] = c.raw
        d = vb.to_device(pad)
        got = vb.analyze_clips(d, lengths, ah._params(pkg), frame_len=N, stride=H)
        _compare(f"padded {fmt}", vb, pkg, got, clips, N, H, "plain")
        d.free()


def test_three_hundred_clips_of_one_to_three_frames(vb, pkg, base):
    N, H = 1200, 480
    rng = np.random.default_rng(300)
    lengths = [int(N + H * rng.integers(0, 3) + rng.integers(0, H)) for _ in range(300)]
    clips = [Clip(base, "pcm16", k, ln) for k, ln in enumerate(lengths)]
    whole = vb.to_device(np.concatenate([c.raw for c in clips]), np.int16)        # (back to back: every sample behind a clip is another clip's)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    ext, track, _ = _form(pkg, "tracked")
    outs = []
    for gf in (64, 0):
        outs.append(vb.analyze_clips([whole.ptr + 2 * int(o) for o in offs], lengths, ah._params(pkg), ext, track, format=CODE["pcm16"],
                                     group_frames=gf, frame_len=N, stride=H, lists=True))
    assert pkg.clips_plan(lengths, N, H, 64)[2] > 5
    _compare("300 clips, group_frames 64", vb, pkg, outs[0], clips, N, H, "tracked")
    _compare("300 clips, one group", vb, pkg, outs[1], clips, N, H, "tracked")
    whole.free()


def test_errors_and_the_empty_batch_write_nothing(vb, pkg, base):
    N, H = 1200, 480
    lengths = [N + 5 * H, N - 1, N + 2 * H]
    clips = [Clip(base, "pcm16", 90 + k, ln) for k, ln in enumerate(lengths)]
    dev = _upload(vb, clips)
    total = pkg.clips_plan(lengths, N, H)[1]
    p, track = ah._params(pkg), _form(pkg, "tracked")[1]
    w = _width(vb, pkg, "tracked")
    ld = w + (w & 1)
    ar = la.Arena(la.DeviceBackend(vb), "vbx_analyze_clips: rejected calls and empty batches")
    ar.output("rec", np.float64, total, 0, ld=ld)                                 # (no writable column: every byte is a canary)
    ar.output("st", np.int32, 3, 0, ld=total)
    ar.output("cand", np.float64, total, 0, ld=8)
    ar.output("count", np.int32, 1, 0, ld=total)
    ar.output("peak", np.float64, 1, 0, ld=total)
    ar.output("index", np.int32, 1, 0, ld=total)
    ar.place()
    po = pkg.PitchTrackOutputs(ar["cand"], ar["count"], ar["peak"], ar["index"])
    sz = C.c_size_t

    def call(ptrs=None, lens=lengths, n=None, fmt=None, params=p, frame_len=N, stride=H, record_ld=ld, rec="rec", null_arrays=False, tk=track):
        ptrs = [d.ptr if d is not None else None for d in dev] if ptrs is None else ptrs
        n = len(lens) if n is None else n
        h_clip, h_len = (C.c_void_p * max(len(ptrs), 1))(*ptrs), (sz * max(len(lens), 1))(*lens)
        f = pkg.ClipFormat.make(CODE["pcm16"]) if fmt is None else fmt
        return vb.L.vbx_analyze_clips(vb.ctx, None if null_arrays else h_clip, None if null_arrays else h_len, n, C.byref(f), frame_len, stride,
                                      None if params is None else C.byref(params), None, None if tk is None else C.byref(tk),
                                      None if rec is None else ar[rec] if isinstance(rec, str) else rec, record_ld, ar["st"], C.byref(po))

    assert call(null_arrays=True) == E_INVALID                                    # a NULL array with n_clips > 0
    assert call(ptrs=[dev[0].ptr, None, None]) == E_INVALID                       # a NULL clip pointer with a length that gives a frame
    assert call(ptrs=[dev[0].ptr + 1, None, dev[2].ptr]) == E_INVALID             # a clip off its element type's alignment
    assert b"alignment" in vb.L.vbx_last_error(vb.ctx)
    assert call(fmt=pkg.ClipFormat.make(0)) == E_INVALID and call(fmt=pkg.ClipFormat.make(6)) == E_INVALID
    assert call(fmt=pkg.ClipFormat(CODE["pcm16"], 1, 0)) == E_INVALID             # reserved
    assert call(fmt=pkg.ClipFormat.make(CODE["pcm16"], 1)) == E_INVALID and call(fmt=pkg.ClipFormat.make(CODE["pcm16"], 63)) == E_INVALID
    assert call(ptrs=[dev[0].ptr] * 2, lens=[1 << 31, 1 << 31], frame_len=1, stride=1) == E_INVALID        # more than 0x7fffffff rows
    # what vbx_analyze_frames_ex_f64 rejects
    assert call(frame_len=0) == E_INVALID and call(stride=0) == E_INVALID and call(frame_len=(1 << 26) + 1, lens=[1 << 27] * 3) == E_INVALID
    assert call(params=None) == E_INVALID and call(rec=None) == E_INVALID and call(rec=ar["rec"] + 8) == E_INVALID
    assert call(record_ld=ld - 2) == E_INVALID and call(record_ld=ld + 1) == E_INVALID
    bad = ah._params(pkg)
    bad.n_est = 7
    assert call(params=bad) == E_INVALID
    bad = ah._params(pkg)
    bad.lpc_order = 2000                                                          # (only the LPC part itself knows: the first group's call)
    assert call(params=bad) == E_INVALID
    bad_tk = pkg.PitchTrackParams.make(kmax=0)
    assert call(tk=bad_tk) == E_INVALID
    # the empty batch and a batch without a frame succeed
    assert call(ptrs=[], lens=[], n=0, null_arrays=True) == 0
    assert call(ptrs=[None, None], lens=[N - 1, 0]) == 0
    ar.finish()                                                                   # ... and nothing was written anywhere
    # the context is usable
    got = _batch(vb, pkg, clips, dev, N, H, "tracked", 0)
    _compare("after the rejected calls", vb, pkg, got, clips, N, H, "tracked")
    for d in dev:
        if d is not None:
            d.free()


@pytest.mark.parametrize("fmt", ["pcm16", "f32"])
def test_launches_do_not_depend_on_the_clip_count(vb, pkg, base, fmt):
    """one group holding 1, 5 and 40 clips of about 120 frames in all: the same kernel names with the same counts, the pack and the
    deliver exactly once each, and at 1200/480 no widening pass (the plane is read as the type it holds)"""
    N, H = 1200, 480
    reports = []
    for lengths in ([N + 119 * H], [N + 23 * H + 11 * k for k in range(5)], [N + 2 * H + 7 * k for k in range(40)]):
        clips = [Clip(base, fmt, 120 + k, ln) for k, ln in enumerate(lengths)]
        dev = _upload(vb, clips)
        assert pkg.clips_plan(lengths, N, H)[2] == 1
        _batch(vb, pkg, clips, dev, N, H, "tracked", 0)                           # (tables and workspaces)
        vb.sync()
        vb.profile(True)
        vb.profile_reset()
        got = _batch(vb, pkg, clips, dev, N, H, "tracked", 0)
        vb.sync()
        reports.append({k: v[1] for k, v in vb.profile_report().items()})
        vb.profile(False)
        _compare(f"profiled, {len(lengths)} clips", vb, pkg, got, clips, N, H, "tracked")
        for d in dev:
            d.free()
    assert reports[0] == reports[1] == reports[2], reports
    r = reports[0]
    assert r["clips_pack_" + fmt] == 1 and r["clips_deliver"] == 1, r
    assert "pcm16" not in r and "f32_to_f64" not in r, r
    assert sum(1 for k in r if k.startswith("clips_pack_")) == 1


def test_a_late_producer_of_the_clips(pkg, vb, base, sctx, hip):  # noqa: F811
    """the clips are produced LATE on the context's (caller-created) stream, with no host wait before the call, and every output is
    consumed on the stream right behind it (tests/stream_harness.py late_producer)"""
    N, H = 1200, 480
    lengths = [N + 30 * H, N - 1, N + 7 * H + 3, N, N + 55 * H + 100]
    clips = [Clip(base, "pcm16", 200 + k, ln) for k, ln in enumerate(lengths)]
    image = np.concatenate([c.raw for c in clips])
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    total = pkg.clips_plan(lengths, N, H)[1]
    c = sctx()
    s = c.vb
    ext, track, _ = _form(pkg, "tracked_ext")
    w = _width(s, pkg, "tracked_ext")
    ld = w + (w & 1)
    x = s.empty(image.size, np.int16)
    rec, st = s.empty((total, ld)), s.empty((3, total), np.int32)
    cand, count, peak, index = s.empty((total, 4, 2)), s.empty(total, np.int32), s.empty(total), s.empty(total, np.int32)

    def call():
        assert s.analyze_clips([x.ptr + 2 * int(o) for o in offs], lengths, ah._params(pkg), ext, track, format=CODE["pcm16"], frame_len=N,
                               stride=H, out=rec, record_ld=ld, status=st, outputs=(cand, count, peak, index)) is None

    r = sh.late_producer(s, c.stream, call, [(x, image)], [rec, st, cand, count, peak, index], c.delay, hip=hip)
    assert r["streams"].get("clips_pack_pcm16") == 0 and r["streams"].get("clips_deliver") == 0, r["streams"]
    _compare("late producer", vb, pkg, r["ref"], clips, N, H, "tracked_ext")


def test_the_c_example_runs(vb, pkg, tmp_path):
    """examples/clip_batch.c: a padded batch of sines of 100 + 40 b Hz through the C ABI from a C program -- every clip with a frame
    is printed with the rows vbx_clips_plan gives it and the median pitch of the resident call on the same samples (to the two
    decimals printed), the two clips shorter than a frame have no rows"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "vox_box.rs_amd", "lib")
    exe = str(tmp_path / "clip_batch")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "clip_batch.c"),
                        "-L", lib, "-lvoxbox_hip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", exe], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], text=True, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    lengths = [48000, 1199, 30001, 1200, 0, 17520]
    rows, total, groups = pkg.clips_plan(lengths, 1200, 480)
    params = pkg.AnalysisParams.make(SR, lpc_order=0, formant_order=0, mfcc=None)           # the example's: pitch only
    for b, ln in enumerate(lengths):
        if rows[b, 1] == 0:
            assert lines[b] == f"clip {b}: {ln} samples, no frame", lines[b]
            continue
        m = re.fullmatch(rf"clip {b}: {ln} samples, rows \[(\d+), (\d+)\), median pitch ([0-9.]+) Hz", lines[b])
        assert m and (int(m.group(1)), int(m.group(2))) == (int(rows[b, 0]), int(rows[b, 0] + rows[b, 1])), lines[b]
        pcm = np.rint(12000.0 * np.sin(2.0 * 3.14159265358979323846 * (100.0 + 40.0 * b) * np.arange(ln, dtype=np.float64) / 48000.0)).astype(np.int16)
        hz = np.sort(vb.analyze_frames_ex_pcm16(pcm, params, frame_len=1200, stride=480)[0][:, 0])
        assert m.group(3) == f"{hz[hz.size // 2]:.2f}", (lines[b], hz[hz.size // 2])
    assert lines[len(lengths)] == f"{total} rows from {groups} group(s)"
