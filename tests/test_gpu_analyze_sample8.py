"""The end-to-end contracts of the 8-bit sample formats on a real MI355X: every byte a call writes for a VBX_SAMPLE_ULAW or ALAW source
equals what the SAME call writes for PCM16 on the decoded int16 samples, and every byte it writes for VBX_SAMPLE_U8 equals what it
writes for F64 on (b - 128) / 127 -- for vbx_analyze_host, vbx_analyze_host_channels, a one-channel and a three-channel live session
(plain, and tracked with the online path bound) and vbx_analyze_clips.  The yardstick is always the other format's run of the same
call (which the existing suites hold to the resident calls), never the 8-bit code against itself, and every comparison is on
integer views of every output array.  The decoded samples come from tests/sample8_cases.py (the ITU formulas restated), not from the
library.  Recordings: the synthetic speech with a stretch of a golden 16-bit WAV, encoded to the nearest codes, with digital silence
(runs of 0xff, of 0xd5, 0x7f / 0xff mixed: all-zero and constant frames) and all 256 codes inside.

Shapes: 400/160; 1200/480, where the decoded int16 plane must take the direct PCM16 kernels (the frame loop's `analyze` launch and no
widening `pcm16` pass); 200/80 at 8 kHz, where the 8-bit call must answer what the PCM16 call answers, whatever that is.  One case
of each call also compares the {profile name: launch count} maps: the mu-law run's equals the PCM16 run's once *_ulaw is read as
*_pcm16 (a mono PCM16 host chunk is read in place, so the host case compares with the stereo PCM16 run)."""
import numpy as np
import pytest

import sample8_cases as s8
import test_gpu_analyze_host as ah
import test_gpu_session_channels_path as scp
import test_gpu_session_path as sp
from sample8_cases import FORMATS8, SAME_AS, TAG, U8, ULAW

pytestmark = pytest.mark.gpu

F = 650
SEG = [0, 150, 200, 390, 600]
_REF = {}


def _u(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind in "iu" else a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def speech(vb, golden_dir):
    """16-bit speech: the synthetic speech with a stretch of the golden WAV in its middle"""
    d = vb.synth_speech(400_000, sample_offset=3 * 48000 + 777)
    x = np.round(d.numpy() * 0.9 * 32767.0).astype(np.int16)
    d.free()
    g = s8.golden_pcm16(golden_dir, "sample-two_vowels.wav")
    m = min(g.size, 60_000)
    x[90_000:90_000 + m] = g[:m]
    return x


def _codes(speech, fmt, n, channels=1, seed=0):
    """[n] or [n, channels] codes: channel c is the recording from another place, with its silence elsewhere"""
    cols = [s8.recording(fmt, n, np.roll(speech, -17_003 * c)[::-1 if c % 2 else 1], seed=seed + c, silent=(0.3 + 0.11 * c, 0.08)) for c in range(channels)]
    return cols[0] if channels == 1 else np.ascontiguousarray(np.stack(cols, axis=1))


def _decoded(fmt, codes):
    return np.ascontiguousarray(s8.decode(fmt, codes).astype(s8.OUT[fmt]))


def _same(label, got, want, width):
    """every array of the two runs, bit for bit; of the records the `width` columns a call writes (an odd record is padded to an even
    leading dimension, and nobody writes the padding)"""
    assert len(got) == len(want), (label, len(got), len(want))
    names = ("records", "status3", "cand", "count", "peak", "index")
    for k, (g, w) in enumerate(zip(got, want)):
        if k == 0:
            assert g.shape == w.shape and g.shape[1] >= width, (label, g.shape, w.shape, width)
            g, w = g[:, :width], w[:, :width]
        ug, uw = _u(g), _u(w)
        assert ug.shape == uw.shape, (label, names[k], ug.shape, uw.shape)
        if names[k] == "cand":                                                   # (entries past a frame's count are not written)
            assert np.array_equal(got[3], want[3]), (label, "count")
            keep = np.arange(g.shape[1])[None, :] < got[3][:, None]
            ug, uw = ug[keep], uw[keep]
        assert np.array_equal(ug, uw), (label, names[k], "first difference at", tuple(np.argwhere(ug != uw)[0]), int((ug != uw).sum()))


def _profiled(vb, fn):
    vb.sync()
    vb.profile(True)
    vb.profile_reset()
    try:
        out = fn()
        vb.sync()
        return out, {k: v[1] for k, v in vb.profile_report().items()}
    finally:
        vb.profile(False)


def _as_pcm16(rep):
    return {(k[:-4] + "pcm16" if k.endswith("_ulaw") else k): v for k, v in rep.items()}


# ---- vbx_analyze_host --------------------------------------------------------------------------------------------------------

def _host(vb, pkg, audio, code, channel, shape, form, seg, chunk, params=None):
    N, H = shape
    ext, track = ah._form(pkg, form)
    return vb.analyze_host(audio, params if params is not None else ah._params(pkg), ext, track, format=code, channel=channel, chunk_frames=chunk,
                           seg_start=seg, frame_len=N, stride=H, lists=track is not None)


def _host_pair(vb, pkg, speech, fmt, channels, shape, form, seg, chunk):
    N, H = shape
    codes = _codes(speech, fmt, (F - 1) * H + N, channels)
    channel = channels - 1
    key = ("host", fmt, channels, shape, form, None if seg is None else tuple(seg), chunk)      # the PCM16 / F64 run: once per case
    if key not in _REF:
        _REF[key] = _host(vb, pkg, _decoded(fmt, codes), None, channel, shape, form, seg, chunk)
    got = _host(vb, pkg, codes, fmt, channel, shape, form, seg, chunk)
    _same(f"analyze_host {TAG[fmt]} {channels}ch {shape} {form} seg {seg} chunk {chunk}", got, _REF[key], ah._width(vb, pkg, form))
    return got


@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo-ch1"])
@pytest.mark.parametrize("form", ["plain", "tracked_ext"])
@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_host_every_cut(vb, pkg, speech, fmt, form, channels):
    for chunk in (64, 200):
        for seg in (None, SEG):
            got = _host_pair(vb, pkg, speech, fmt, channels, (400, 160), form, seg, chunk)
    assert got[0].shape[0] == F and np.isfinite(got[0][:, 2:]).any()


@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_host_takes_the_direct_pcm16_kernels_at_1200(vb, pkg, speech, fmt):
    """1200/480: a G.711 chunk's int16 plane is read by the 1200-sample PCM16 kernels directly (vbx_analyze_frames_pcm16's rule)"""
    for channels in (1, 2):
        _, rep = _profiled(vb, lambda: _host_pair(vb, pkg, speech, fmt, channels, (1200, 480), "plain", None, 200))
        # (_host_pair may run the reference too: the names below are the 8-bit run's or shared by both)
        assert rep.get("unpack_" + TAG[fmt], 0) == 4, rep                        # one unpack per chunk, F = 650 at 200 frames a chunk
    codes = _codes(speech, fmt, (F - 1) * 480 + 1200, 1)
    _, rep = _profiled(vb, lambda: _host(vb, pkg, codes, fmt, 0, (1200, 480), "plain", None, 200))
    assert "analyze" in rep and rep["unpack_" + TAG[fmt]] == 4, rep
    if fmt != U8:
        assert "pcm16" not in rep and "f32_to_f64" not in rep, ("a widening pass ran in front of the frame loop", sorted(rep))
    assert not [k for k in rep if k.startswith("unpack_") and k != "unpack_" + TAG[fmt]], sorted(rep)


def test_host_launch_counts_are_pcm16s(vb, pkg, speech):
    """the same launches per chunk for mu-law as for PCM16: mono mu-law against channel 1 of stereo PCM16 (a mono PCM16 chunk is read in
    place and launches no unpack), and stereo against stereo"""
    for shape in ((400, 160), (1200, 480)):
        N, H = shape
        stereo = _codes(speech, ULAW, (F - 1) * H + N, 2)
        mono = np.ascontiguousarray(stereo[:, 1])                                # (the same samples: what is launched may depend on them)
        _, r_mono = _profiled(vb, lambda: _host(vb, pkg, mono, ULAW, 0, shape, "tracked_ext", SEG, 200))
        _, r_st = _profiled(vb, lambda: _host(vb, pkg, stereo, ULAW, 1, shape, "tracked_ext", SEG, 200))
        _, r_ref = _profiled(vb, lambda: _host(vb, pkg, _decoded(ULAW, stereo), None, 1, shape, "tracked_ext", SEG, 200))
        assert "unpack_pcm16" in r_ref and _as_pcm16(r_mono) == r_ref and _as_pcm16(r_st) == r_ref, (shape, r_mono, r_st, r_ref)


@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_host_200_80_at_8khz_answers_what_pcm16_answers(vb, pkg, speech, fmt):
    p = pkg.AnalysisParams.make(8000.0, pitch=(0.2, 75.0, 500.0), mfcc=(13, 100.0, 3800.0))
    codes = _codes(speech, fmt, (F - 1) * 80 + 200, 1)

    def run(audio, code):
        try:
            return _host(vb, pkg, audio, code, 0, (200, 80), "plain", SEG, 200, params=p)
        except pkg.VoxBoxError as e:
            return str(e)
    want, got = run(_decoded(fmt, codes), None), run(codes, fmt)
    assert isinstance(got, str) == isinstance(want, str), (got if isinstance(got, str) else "accepted", want if isinstance(want, str) else "accepted")
    if isinstance(want, str):
        assert got == want
    else:
        _same(f"analyze_host {TAG[fmt]} 200/80 at 8 kHz", got, want, ah._width(vb, pkg, "plain"))


@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_host_lpc_policy_reference(vb, pkg, speech, fmt, request):
    old = vb.lpc_policy
    request.addfinalizer(lambda: setattr(vb, "lpc_policy", old))
    vb.lpc_policy = pkg.LPC_POLICY_REFERENCE
    codes = _codes(speech, fmt, (F - 1) * 160 + 400, 2)
    want = _host(vb, pkg, _decoded(fmt, codes), None, 1, (400, 160), "tracked_ext", SEG, 64)
    _same(f"analyze_host {TAG[fmt]} LPC_POLICY_REFERENCE", _host(vb, pkg, codes, fmt, 1, (400, 160), "tracked_ext", SEG, 64), want,
          ah._width(vb, pkg, "tracked_ext"))


# ---- vbx_analyze_host_channels -----------------------------------------------------------------------------------------------

def _host_channels(vb, pkg, audio, code, shape, form, seg, chunk):
    N, H = shape
    ext, track = ah._form(pkg, form)
    return vb.analyze_host_channels(audio, ah._params(pkg), ext, track, format=code, select=[3, 0, 2], chunk_frames=chunk, seg_start=seg,
                                    frame_len=N, stride=H, lists=track is not None)


@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_host_channels_three_of_four(vb, pkg, speech, fmt):
    reps = {}
    for shape, form, seg, chunk in (((400, 160), "tracked_ext", SEG, 64), ((400, 160), "plain", None, 200), ((1200, 480), "tracked_ext", SEG, 200)):
        N, H = shape
        codes = _codes(speech, fmt, (F - 1) * H + N, 4)
        want, reps["ref"] = _profiled(vb, lambda: _host_channels(vb, pkg, _decoded(fmt, codes), None, shape, form, seg, chunk))
        got, reps["got"] = _profiled(vb, lambda: _host_channels(vb, pkg, codes, fmt, shape, form, seg, chunk))
        assert len(got) == len(want) == 3
        for k in range(3):
            _same(f"analyze_host_channels {TAG[fmt]} {shape} {form} plane {k}", got[k], want[k], ah._width(vb, pkg, form))
        assert _u(got[0][0]).tobytes() != _u(got[1][0]).tobytes()                # (the channels differ: no plane mix-up can pass)
        assert reps["got"]["unpack_all_" + TAG[fmt]] == -(-F // chunk), reps["got"]
        if fmt == ULAW:
            assert _as_pcm16(reps["got"]) == reps["ref"], (shape, form, reps)
        if fmt != U8 and shape == (1200, 480):
            assert "analyze" in reps["got"] and "pcm16" not in reps["got"], sorted(reps["got"])


# ---- live sessions -----------------------------------------------------------------------------------------------------------

SN, SH = 400, 160
ST = (sp.F - 1) * SH + SN
_HEAD = [1, SH - 1, SH, 3 * SH + 7]
_MID = ((100 - 1) * SH + SN) - sum(_HEAD)                                        # the fifth block ends where frame 100 does: the mark
SIZES = _HEAD + [_MID, ST - sum(_HEAD) - _MID]
MARKS = (100,)


def _session_plain(vb, pkg, audio, code, channels, select):
    """every push's returned arrays, a mark in the middle; select None: a one-channel session on the last channel"""
    p = sp._params(pkg)
    kw = dict(format=code, channels=channels, frame_len=SN, stride=SH, max_block=max(SIZES))
    sess = vb.session(p, None, None, channel=channels - 1, **kw) if select is None else vb.session_channels(p, None, None, select=select, **kw)
    outs, pos = [], 0
    with sess:
        for n in SIZES:
            if sess.info()[1] in MARKS:
                sess.mark_utterance()
            r = sess.push(audio[pos:pos + n])
            outs += list(r) if select is None else [a for per in r for a in per]
            pos += n
        assert sess.info()[1] == sp.F
    return outs


def _session_bound(vb, pkg, audio, code, channels, select, kmax=4):
    """tracked, the online path bound: every array every push and mark writes, in canary-filled buffers (tests/test_gpu_session_path.py)"""
    p, track = sp._params(pkg), sp._track(pkg, kmax, 0.0)
    n_slots, rows = len(SIZES) + len(MARKS) + 1, sp.MP + max(SIZES) // SH + 2
    runs = [sp.Run(vb, pkg, kmax, n_slots, rows) for _ in (select if select is not None else [0])]
    kw = dict(format=code, channels=channels, frame_len=SN, stride=SH, max_block=max(SIZES))
    try:
        if select is None:
            with vb.session(p, None, track, channel=channels - 1, **kw) as sess:
                slots = scp._feed(sess, runs, audio, SIZES, MARKS, 1.0, sp.MP, multi=False)
        else:
            with vb.session_channels(p, None, track, select=select, **kw) as sess:
                slots = scp._feed(sess, runs, audio, SIZES, MARKS, 1.0, sp.MP, multi=True)
        vb.sync()
        return [d.numpy() for x in runs for d in x.all], slots
    finally:
        for x in runs:
            x.free()


@pytest.mark.parametrize("channels,select", [(1, None), (2, None), (4, [3, 0, 2])], ids=["mono", "stereo-ch1", "three-of-four"])
@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_sessions(vb, pkg, speech, fmt, channels, select):
    codes = _codes(speech, fmt, ST, channels, seed=40)
    ref = _decoded(fmt, codes)
    want, r_ref = _profiled(vb, lambda: _session_plain(vb, pkg, ref, SAME_AS[fmt], channels, select))
    got, r_got = _profiled(vb, lambda: _session_plain(vb, pkg, codes, fmt, channels, select))
    assert len(got) == len(want) and sum(a.shape[0] for a in got[0::2]) == sp.F * (1 if select is None else 3)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and _u(g).tobytes() == _u(w).tobytes(), (TAG[fmt], channels, select, "plain, returned array", k)
    name = ("session_ingest_" if select is None else "session_ingest_all_") + TAG[fmt]
    assert r_got[name] == len(SIZES), r_got                                       # one ingest launch per push
    if fmt == ULAW:
        assert _as_pcm16(r_got) == r_ref, (r_got, r_ref)
    (want, s_ref), (got, s_got) = _session_bound(vb, pkg, ref, SAME_AS[fmt], channels, select), _session_bound(vb, pkg, codes, fmt, channels, select)
    assert s_ref == s_got and len(got) == len(want)
    names = ("records", "status3", "cand", "count", "peak", "path", "index", "forced", "commit")
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), (TAG[fmt], channels, select, "bound, plane", k // 9, names[k % 9])
    assert int(got[8][:s_got, 1].sum()) == sp.F                                  # every row of the contour was committed


# ---- vbx_analyze_clips -------------------------------------------------------------------------------------------------------

def _clip_lengths(N, H):
    ls = [N + 70 * H + 1, N, N - 1, N + H // 2, N + H // 2 + 1, N + H, 0, N + 150 * H, N + 3 * H + 7, N + 20 * H, 1, H - 1, H + 1, 3000 + H // 2]
    return ls + [N + ((7 * k) % 23) * H + (13 * k) % H for k in range(40 - len(ls))]


def _clips(vb, pkg, dev, offs, lengths, code, itemsize, shape, form, gf):
    N, H = shape
    ext, track = ah._form(pkg, form)
    return vb.analyze_clips([dev.ptr + int(o) * itemsize for o in offs], lengths, ah._params(pkg), ext, track, format=code, group_frames=gf,
                            frame_len=N, stride=H, lists=track is not None)


@pytest.mark.parametrize("shape", [(400, 160), (1200, 480)], ids=["400-160", "1200-480"])
@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_clips_forty_ragged(vb, pkg, speech, fmt, shape):
    N, H = shape
    lengths = _clip_lengths(N, H)
    assert len(lengths) == 40
    # the clips lie back to back in one buffer, one poison byte between them: most start at odd byte addresses
    offs = np.concatenate([[0], np.cumsum([ln + 1 for ln in lengths])[:-1]])
    codes = _codes(speech, fmt, int(offs[-1]) + lengths[-1] + 1, 1, seed=90)
    ref = _decoded(fmt, codes)
    d_codes, d_ref = vb.to_device(codes, np.uint8), vb.to_device(ref)
    try:
        for form, gf in (("tracked_ext", 64), ("tracked_ext", 0), ("plain", 64)):
            want, r_ref = _profiled(vb, lambda: _clips(vb, pkg, d_ref, offs, lengths, SAME_AS[fmt], ref.dtype.itemsize, shape, form, gf))
            got, r_got = _profiled(vb, lambda: _clips(vb, pkg, d_codes, offs, lengths, fmt, 1, shape, form, gf))
            _same(f"analyze_clips {TAG[fmt]} {shape} {form} group_frames {gf}", got, want, ah._width(vb, pkg, form))
            groups = pkg.clips_plan(lengths, N, H, gf)[2]
            assert r_got["clips_pack_" + TAG[fmt]] == groups and r_got["clips_deliver"] == groups, r_got
            assert sum(1 for k in r_got if k.startswith("clips_pack_")) == 1 and not [k for k in r_got if k.startswith("unpack")], sorted(r_got)
            if fmt == ULAW:
                assert _as_pcm16(r_got) == r_ref, (r_got, r_ref)
            if fmt != U8 and shape == (1200, 480):
                assert "analyze" in r_got and "pcm16" not in r_got and "f32_to_f64" not in r_got, sorted(r_got)
    finally:
        d_codes.free(); d_ref.free()


def test_rejections(vb, pkg, speech):
    codes = _codes(speech, ULAW, 4000, 1)
    p = ah._params(pkg)
    for bad in (0, 6, 7, 15, 19):
        with pytest.raises(pkg.VoxBoxError):
            vb.analyze_host(codes.ctypes.data, p, format=bad, channels=1, n_sample_frames=4000, frame_len=400, stride=160)
        with pytest.raises(pkg.VoxBoxError):
            vb.session(p, format=bad, frame_len=400, stride=160)
        with pytest.raises(pkg.VoxBoxError):
            vb.session_channels(p, format=bad, channels=2, frame_len=400, stride=160)
        d = vb.to_device(codes, np.uint8)
        with pytest.raises(pkg.VoxBoxError):
            vb.analyze_clips([d.ptr], [4000], p, format=bad, frame_len=400, stride=160)
        d.free()
    # an 8-bit format is never inferred and never taken with another array type
    with pytest.raises(AssertionError):
        vb.analyze_host(codes.astype(np.int16), p, format=ULAW, frame_len=400, stride=160)
    got = vb.analyze_host(codes, p, format=ULAW, frame_len=400, stride=160)      # the context is usable afterwards
    assert got[0].shape[0] == (4000 - 400) // 160 + 1


def test_the_c_example_runs(vb, tmp_path):
    """examples/telephone_clips.c without a file: twelve seconds of a gliding tone, encoded to mu-law with vbx_g711_table, cut into
    2.5 s clips and analysed at 200 / 80 by ONE vbx_analyze_clips call on the bytes.  Checked here: the program's own bookkeeping --
    the clips, their frame counts, the rows and groups of the plan -- and that every clip reports a pitch inside the limits it asked
    for.  (What the numbers ARE is the contract tests' business: bit for bit the PCM16 call's.  A first version of this test held
    each median to 2 Hz of the glide; at 8 kHz one sample of lag is 3 Hz at 157 Hz, and the clip around 157 Hz gave 153.85 Hz =
    8000 / 52 -- that bound was wrong about the estimator's resolution, not a finding about the 8-bit path.)"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib, exe = os.path.join(root, "vox_box.rs_amd", "lib"), str(tmp_path / "telephone_clips")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "telephone_clips.c"),
                        "-L", lib, "-lvoxbox_hip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", exe], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], text=True, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = re.findall(r"clip (\d+): (\d+) samples, (\d+) frames, median pitch ([0-9.]+) Hz", r.stdout)
    assert [(int(k), int(n)) for k, n, _, _ in rows] == [(0, 20000), (1, 20000), (2, 20000), (3, 20000), (4, 16000)], r.stdout
    for k, n, frames, hz in rows:
        assert int(frames) == (int(n) - 200) // 80 + 1 and 75.0 <= float(hz) <= 500.0, (k, n, frames, hz)
    assert "mu-law at 8000 Hz: 1190 rows from 1 group(s)" in r.stdout, r.stdout
