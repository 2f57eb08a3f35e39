"""The frame loop's dispatch by sample type, pinned to the build BEFORE the sample type became one tagged view (frames_t,
vbx_kernels.hpp): which launches a call makes, how often, on which stream, and what they write.

Every cell is one small call with profiling on.  A cell holds
  * {profile name: [launch count, stream id]} (vbx_profile_names / _get / _stream),
  * the sha-256 of the records (their own columns, not the padding up to an even record_ld) and of status3,
  * in tracked cells also the sha-256 of count and index.
The cells are the product of
  kind    f64, pcm16, f32 (float32 has only the _ex entry point: the plain and tracked forms pass a null extension)
  shape   1200/480 (the native fused shape: no widening pass), 1024/512 (fused, widened), 400/160 (below SPECTRAL_MIN_N: run_pitch
          alone, LPC and MFCC beside it), 5000/2500 (beyond VBX_MAX_FRAME_LEN: one stream; 3 frames)
  form    plain; tracked A (kmax 4, a silence threshold: the frame_peak* kernels); tracked B (no threshold, no peak output: no peak
          kernel); _ex direct (ratio 0.25 with RMS); _ex tracked with RMS (the frame_rms_peak fusion); and _ex dense fallback, at
          4096/2048 with ratio 0.5 in place of the shape column
  lpc     12 (LPC joins the fused kernel), 10 (LPC beside it)
with MFCC at 13 coefficients and formants at order 12 everywhere; plus vbx_analyze_host on a mono PCM16 and on a stereo F32 recording
(two chunks each: the no-unpack slot path and the typed-plane path of its decode) and one session push (the session's decode).

The per-type launchers with names of their own are what a dispatch slip would swap silently -- frame_peak / frame_peak_pcm16 /
frame_peak_f32in, burg_lags / burg_lags_resampled, pcm16 / f32_to_f64 -- and what this test exists to catch.

tests/golden/frames_dispatch.json is recorded on the PARENT commit's library by tools/record_frames_dispatch.py, never on the
code under test.

Needs a real MI355X: run with `-m gpu`.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 48000.0
OFFSET = 3 * 48000 + 12345
FRAMES = 40
SHAPES = [(1200, 480, FRAMES), (1024, 512, FRAMES), (400, 160, FRAMES), (5000, 2500, 3)]
DENSE = (4096, 2048, FRAMES)                                 # ratio 0.5: m = 2048, the dense fallback (tests/test_gpu_analyze_ex.py)
KINDS = ("f64", "pcm16", "f32")
FORMS = ("plain", "tracked A", "tracked B", "ex direct", "ex tracked rms")
LPC_ORDERS = (12, 10)
HOST_FRAMES, HOST_CHUNK = 100, 64                            # two chunks at the smallest chunk_frames (VBX_SHARD_WARM_FRAMES)
GOLDEN = "frames_dispatch.json"


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _samples(x, kind):
    """the synth fixture's samples as the kind's own type: rounded to int16 for PCM, to float32 for float"""
    if kind == "pcm16":
        return np.clip(np.rint(x * 20000.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32) if kind == "f32" else x


def _params(pkg, lpc_order):
    est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    return pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=lpc_order, formant_order=12, est_init=est0,
                                   mfcc=(13, 100.0, 8000.0))


def _form(pkg, form):
    """-> (ext, track, with a peak output)"""
    if form == "plain":
        return None, None, False
    if form == "tracked A":
        return None, pkg.PitchTrackParams.make(kmax=4, silence_threshold=0.03), True
    if form == "tracked B":
        return None, pkg.PitchTrackParams.make(kmax=4, silence_threshold=0.0), False
    if form == "ex direct":
        return pkg.AnalysisExt.make(0.25, rms=True), None, False
    if form == "ex tracked rms":
        return pkg.AnalysisExt.make(0.0, rms=True), pkg.PitchTrackParams.make(kmax=4, silence_threshold=0.03), True
    assert form == "ex dense"
    return pkg.AnalysisExt.make(0.5), None, False


def _profiled(vb, call):
    vb.profile_reset()
    vb.profile(True)
    try:
        res = call()
        rep, streams = vb.profile_report(), vb.profile_streams()
    finally:
        vb.profile(False)
    return res, {name: [int(rep[name][1]), int(streams[name])] for name in sorted(rep)}


def _cell(launches, width, rec, st3, count=None, index=None):
    d = {"launches": launches, "records": _sha(rec[:, :width]), "status3": _sha(st3)}
    if count is not None:
        d["count"] = _sha(count)
    if index is not None:
        d["index"] = _sha(index)
    return d


def _width(vb, params, ext):
    return int(vb.L.vbx_record_doubles_ex(C.byref(params), None if ext is None else C.byref(ext)))


def _resident_cell(vb, pkg, kind, x_d, n, hop, frames, form, lpc_order):
    params = _params(pkg, lpc_order)
    ext, track, with_peak = _form(pkg, form)
    kw = dict(frame_len=n, stride=hop, n_frames=frames)
    own = []
    if track is not None:
        own = [vb.empty((frames, 4, 2)), vb.empty(frames, np.int32), vb.empty(frames) if with_peak else None, vb.empty(frames, np.int32)]
        kw["outputs"] = tuple(own)
    # the entry point the form names; float32 exists only as _ex_f32in
    if kind == "f32":
        call = lambda: vb.analyze_frames_ex_f32in(x_d, params, ext, track, **kw)
    elif form.startswith("ex"):
        fn = vb.analyze_frames_ex_pcm16 if kind == "pcm16" else vb.analyze_frames_ex
        call = lambda: fn(x_d, params, ext, track, **kw)
    elif track is not None:
        fn = vb.analyze_frames_tracked_pcm16 if kind == "pcm16" else vb.analyze_frames_tracked
        call = lambda: fn(x_d, params, track, **kw)
    else:
        fn = vb.analyze_frames_pcm16 if kind == "pcm16" else vb.analyze_frames
        call = lambda: fn(x_d, params, **kw)
    try:
        (rec, st3), launches = _profiled(vb, call)
        count = own[1].numpy() if own else None
        index = own[3].numpy() if own else None
    finally:
        for d in own:
            if d is not None:
                d.free()
    return _cell(launches, _width(vb, params, ext), rec, st3, count, index)


def compute_cells(vb, pkg):
    """{cell name: {"launches": {profile name: [launch count, stream id]}, "records": sha, "status3": sha[, "count", "index"]}}"""
    total = max((f - 1) * hop + n for n, hop, f in SHAPES + [DENSE])
    total = max(total, (HOST_FRAMES - 1) * 480 + 1200)
    d = vb.synth_speech(total, sample_offset=OFFSET)
    x = d.numpy()
    d.free()
    cells = {}
    for kind in KINDS:
        s = _samples(x, kind)
        x_d = vb.to_device(s, s.dtype)
        try:
            for lpc_order in LPC_ORDERS:
                for n, hop, frames in SHAPES:
                    for form in FORMS:
                        cells["%s %d/%d %s lpc%d" % (kind, n, hop, form, lpc_order)] = _resident_cell(vb, pkg, kind, x_d, n, hop, frames, form, lpc_order)
                n, hop, frames = DENSE
                cells["%s %d/%d ex dense lpc%d" % (kind, n, hop, lpc_order)] = _resident_cell(vb, pkg, kind, x_d, n, hop, frames, "ex dense", lpc_order)
        finally:
            x_d.free()
    # host-resident recordings: mono PCM16 is read from the upload slot itself, a stereo F32 one is unpacked into a typed plane
    n, hop = 1200, 480
    t_host = (HOST_FRAMES - 1) * hop + n
    params = _params(pkg, 12)
    ext = pkg.AnalysisExt.make(0.25, rms=True)
    track = pkg.PitchTrackParams.make(kmax=4, silence_threshold=0.03)
    width = _width(vb, params, ext)
    mono = _samples(x[:t_host], "pcm16")
    stereo = np.stack([_samples(x[:t_host], "f32")[::-1], _samples(x[:t_host], "f32")], axis=1)
    for name, audio, channel in (("host pcm16 mono", mono, 0), ("host f32 stereo ch1", stereo, 1)):
        (rec, st3, _cand, count, _peak, index), launches = _profiled(
            vb, lambda: vb.analyze_host(audio, params, ext, track, channel=channel, chunk_frames=HOST_CHUNK, frame_len=n, stride=hop, lists=True))
        cells[name] = _cell(launches, width, rec, st3, count, index)
    # a live session: one push of FRAMES frames of float32 samples, tracked with RMS
    block = _samples(x[:(FRAMES - 1) * hop + n], "f32")
    with vb.session(params, ext, track, format=pkg.SAMPLE_F32, frame_len=n, stride=hop, max_block=block.size) as ses:
        (rec, st3, _cand, count, _peak), launches = _profiled(vb, lambda: ses.push(block))
    cells["session f32 push"] = _cell(launches, width, rec, st3, count)
    return cells


_CELLS = {}


def _cells_cached(vb, pkg):
    if not _CELLS:
        _CELLS.update(compute_cells(vb, pkg))
    return _CELLS


def test_every_cell_of_the_product_is_there(vb, pkg):
    cells = _cells_cached(vb, pkg)
    assert len(cells) == len(KINDS) * len(LPC_ORDERS) * (len(SHAPES) * len(FORMS) + 1) + 3
    # what each shape and form is there for, read off the f64 / PCM / float cells themselves
    for kind, widen, peak in (("pcm16", "pcm16", "frame_peak_pcm16"), ("f32", "f32_to_f64", "frame_peak_f32in"), ("f64", None, "frame_peak")):
        native = cells["%s 1200/480 tracked A lpc12" % kind]["launches"]
        assert "analyze" in native and "pcm16" not in native and "f32_to_f64" not in native, (kind, sorted(native))
        assert peak in native and len([k for k in native if k.startswith("frame_peak")]) == 1, (kind, sorted(native))
        assert not [k for k in cells["%s 1200/480 tracked B lpc12" % kind]["launches"] if k.startswith("frame_peak")]
        assert "frame_rms_peak" in cells["%s 1200/480 ex tracked rms lpc12" % kind]["launches"]
        assert "burg_lags_resampled" in cells["%s 1200/480 ex direct lpc12" % kind]["launches"]
        assert "resample" in cells["%s 4096/2048 ex dense lpc12" % kind]["launches"]
        for name in ("%s 1024/512 plain lpc12", "%s 1200/480 plain lpc10", "%s 400/160 plain lpc12", "%s 5000/2500 plain lpc12", "%s 4096/2048 ex dense lpc12"):
            got = cells[name % kind]["launches"]
            assert (widen in got) if widen else ("pcm16" not in got and "f32_to_f64" not in got), (name % kind, sorted(got))
        assert "analyze" not in cells["%s 400/160 plain lpc12" % kind]["launches"]
        assert set(v[1] for v in cells["%s 5000/2500 plain lpc12" % kind]["launches"].values()) == {0}


def test_dispatch_keeps_the_parent_builds_launches_and_digests(vb, pkg, golden_dir):
    with open(os.path.join(golden_dir, GOLDEN)) as f:
        want = json.load(f)["cells"]
    got = _cells_cached(vb, pkg)
    assert sorted(got) == sorted(want)                       # no cell missing, none unknown
    differ = []
    for name in sorted(want):
        w, g = want[name], got[name]
        if sorted(w) != sorted(g):
            differ.append("%s: keys %s != %s" % (name, sorted(g), sorted(w)))
            continue
        if g["launches"] != w["launches"]:                   # a dict compare: a name missing on either side differs
            only_g = sorted(set(g["launches"]) - set(w["launches"])); only_w = sorted(set(w["launches"]) - set(g["launches"]))
            moved = sorted(k for k in set(g["launches"]) & set(w["launches"]) if g["launches"][k] != w["launches"][k])
            differ.append("%s: launches only here %s, only in the golden %s, count / stream differs %s" % (name, only_g, only_w, moved))
        differ += ["%s: %s" % (name, k) for k in sorted(w) if k != "launches" and g[k] != w[k]]
    assert not differ, "\n".join(differ)
