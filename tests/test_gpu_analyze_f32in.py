"""vbx_analyze_frames_ex_f32in and vbx_f32_to_f64 on a real MI355X: the fused frame loop on float32 samples.  Every comparison
is BIT FOR BIT (uint64 / uint32 views, so NaN payloads count) against the library's own f64 call on the exactly widened samples
-- x32.astype(float64) on the host -- over every frame: no tolerance is needed, because widening a float is exact.  Shapes:
1200 / 480 reads the floats directly (no f64 copy exists); every other shape is widened first into a context-owned copy."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import layout_arena as la

pytestmark = pytest.mark.gpu

SR = 48000.0
N0, H0 = 1200, 480
E_INVALID = -1
WIDEN = "f32_to_f64"                       # the widening kernel's profile name


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _params(pkg, **kw):
    kw.setdefault("est_init", np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES]))
    return pkg.AnalysisParams.make(SR, **kw)


def _width(vb, params, ext):
    return int(vb.L.vbx_record_doubles_ex(C.byref(params), None if ext is None else C.byref(ext)))


def _probes(vb):
    return (vb.last_unsure_count(), vb.last_burg_direct_count(), vb.last_lpc_exact_count(), vb.last_path_chunks_redone())


def _call(vb, fn, x, params, ext, track, N, H, F, seg=None):
    """(records [F, width], status3, lists or (), probes) of one call"""
    got = fn(x, params, ext, track, seg_start=seg, frame_len=N, stride=H, n_frames=F, lists=track is not None)
    return got[0][:, :_width(vb, params, ext)], got[1], tuple(got[2:]), _probes(vb)


def _assert_same(label, got, want, kmax=0):
    rec, st, lists, probes = got
    wrec, wst, wlists, wprobes = want
    assert rec.shape == wrec.shape, (label, rec.shape, wrec.shape)
    a, b = _u64(rec), _u64(wrec)
    assert np.array_equal(a, b), (label, "records: first differing (frame, column)", tuple(np.argwhere(a != b)[0]), int((a != b).sum()))
    assert np.array_equal(st, wst), (label, "status3", np.argwhere(st != wst)[:8])
    assert probes == wprobes, (label, "unsure / burg direct / lpc exact / path chunks redone", probes, wprobes)
    assert len(lists) == len(wlists)
    if lists:
        cand, count, peak, index = lists
        wcand, wcount, wpeak, windex = wlists
        assert np.array_equal(count, wcount) and np.array_equal(index, windex), label
        assert np.array_equal(_u64(peak), _u64(wpeak)), (label, "peak", np.argwhere(_u64(peak) != _u64(wpeak))[:8])
        keep = np.arange(cand.shape[1])[None, :] < count[:, None]             # (entries past a frame's count are not written)
        assert np.array_equal(_u64(cand)[keep], _u64(wcand)[keep]), (label, "candidate lists")


def _both(vb, label, x32, params, ext, track, N, H, F=None, seg=None):
    """the float call against analyze_frames_ex on the widened samples; returns the float call's results"""
    F = vb.L.vbx_frame_count(x32.size, N, H) if F is None else F
    x64 = x32.astype(np.float64)
    want = _call(vb, vb.analyze_frames_ex, x64, params, ext, track, N, H, F, seg)
    got = _call(vb, vb.analyze_frames_ex_f32in, x32, params, ext, track, N, H, F, seg)
    _assert_same(label, got, want)
    return got, want


@pytest.fixture(scope="module")
def synth32(vb):
    d = vb.synth_speech(4 * 48000, sample_offset=3 * 48000 + 12345)
    h = d.numpy()
    d.free()
    return h.astype(np.float32)


@pytest.fixture(scope="module")
def wav32(golden_dir):
    with wave.open(os.path.join(golden_dir, "sample-two_vowels.wav"), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return (pcm.astype(np.float64) / 32767.0).astype(np.float32)


@pytest.fixture
def policy(vb, pkg):
    old = vb.lpc_policy

    def set_policy(name):
        vb.lpc_policy = getattr(pkg, "LPC_POLICY_" + name)
    yield set_policy
    vb.lpc_policy = old


def test_f32_to_f64_is_exact(vb, synth32):
    x = synth32[:50001].copy()
    x[:6] = [1e-40, -0.0, np.inf, -np.inf, np.nan, np.finfo(np.float32).max]
    assert np.float32(1e-40).astype(np.float64) != 0.0
    for n in (50001, 50000, 1, 2, 3):
        d = vb.f32_to_f64(x[:n])
        got = d.numpy()
        d.free()
        assert np.array_equal(_u64(got), _u64(x[:n].astype(np.float64))), n
    # source and destination at the other residues: the pairs are formed from the destination's alignment
    xd, od = vb.to_device(x, np.float32), vb.empty(50001 + 2)
    for so, do in ((0, 1), (1, 0), (1, 1), (3, 1)):
        n = 40001
        vb._check(vb.L.vbx_f32_to_f64(vb.ctx, xd.ptr + 4 * so, n, od.ptr + 8 * do))
        got = od.numpy()[do:do + n]
        assert np.array_equal(_u64(got), _u64(x[so:so + n].astype(np.float64))), (so, do)
    assert vb.L.vbx_f32_to_f64(vb.ctx, None, 0, None) == 0 and vb.L.vbx_f32_to_f64(vb.ctx, None, 4, od.ptr) == E_INVALID
    xd.free(); od.free()


# ---- 1. the native shape, all parts on ---------------------------------------------------------------------------------------------

FORMS = ["plain", "tracked", "ext250", "ext300", "order11"]


@pytest.mark.parametrize("pol", ["EXACT", "REFERENCE"])
@pytest.mark.parametrize("form", FORMS)
def test_native_shape_is_the_f64_call_bit_for_bit(vb, pkg, synth32, wav32, policy, form, pol):
    policy(pol)
    F = 300                                                    # more than one 256-frame path chunk
    params = _params(pkg, formant_order=11 if form == "order11" else 12)
    ext = {"ext250": pkg.AnalysisExt.make(10000.0 / 48000.0, rms=True), "ext300": pkg.AnalysisExt.make(0.25, rms=True)}.get(form)
    track = pkg.PitchTrackParams.make(kmax=4) if form == "tracked" else None
    if ext is not None:
        assert int(vb.L.vbx_resampled_len(N0, ext.formant_resample_ratio)) == (250 if form == "ext250" else 300)
    vb.profile(True)
    vb.profile_reset()
    try:
        for name, sig in (("synth", synth32), ("wav", wav32)):
            n = min(F, int(vb.L.vbx_frame_count(sig.size, N0, H0)))
            x32 = sig[:(n - 1) * H0 + N0]
            got, want = _both(vb, f"{form} {pol} {name}", x32, params, ext, track, N0, H0, n)
            if form == "order11":
                assert got[3][1] == -1                         # no one-pass form at order 11: every frame through the direct kernel
            elif form == "ext250":
                assert got[3][1] == -1                         # m = 250: the direct resampled loader
            else:
                assert got[3][1] >= 0                          # the one-pass lag kernels (m = 300: on the resampled view)
        # native means no copy: the widening kernel did not run (the f64 reference calls never run it either)
        assert WIDEN not in vb.profile_report(), sorted(vb.profile_report())
    finally:
        vb.profile(False)


# ---- 2. the list kernels are reached ------------------------------------------------------------------------------------------------

def _mixed_recording(wav32):
    F = 160
    x = np.zeros((F - 1) * H0 + N0, dtype=np.float32)
    rng = np.random.default_rng(7)
    for pos in (1500, 2100, 2700, 5000, 5300, 7100):           # a few impulses in silence: lag curves that are exactly zero over stretches
        x[pos] = rng.uniform(0.5, 1.0)
    t = np.arange(9600)
    x[9600:19200] = (0.5 * np.sin(2.0 * np.pi * 440.0 * t / SR)).astype(np.float32)       # a pure tone
    x[19200:28800] = 0.25                                                                  # DC
    # [28800, 38400): silence
    x[38400:38400 + 29520] = wav32[:29520]                     # frames 0..59 of the recording, on the frame grid (38400 = 80 hops)
    x[67920:] = (0.1 * rng.standard_normal(x.size - 67920)).astype(np.float32)
    return x, F


@pytest.mark.parametrize("tracked", [False, True])
def test_list_kernels_are_reached_and_agree(vb, pkg, wav32, tracked):
    x32, F = _mixed_recording(wav32)
    params = _params(pkg)
    track = pkg.PitchTrackParams.make(kmax=4) if tracked else None
    got, want = _both(vb, "mixed", x32, params, None, track, N0, H0, F)
    unsure, burg_direct, lpc_exact, _ = want[3]
    assert unsure > 0 and burg_direct > 0 and lpc_exact > 0, want[3]       # (the speech stretch: rows 14, 31, 41, 48 by tests/lpc_exact_model.py)
    assert got[3] == want[3]


# ---- 3. special values --------------------------------------------------------------------------------------------------------------

def test_special_values_arrive_as_they_are(vb, pkg, synth32):
    F = 40
    x32 = synth32[:(F - 1) * H0 + N0].copy()
    specials = {4: np.float32(1e-40), 10: np.float32(-0.0), 16: np.float32(np.inf), 22: np.float32(np.nan),
                28: np.finfo(np.float32).max}
    for t, v in specials.items():
        x32[t * H0 + 700] = v                                  # (sample 700 of frame t is sample 220 of frame t + 1: both are compared)
    assert np.float32(1e-40).astype(np.float64) != 0.0         # the host conversion does not flush either
    params = _params(pkg)
    ext = pkg.AnalysisExt.make(0.25, rms=True)
    for track in (None, pkg.PitchTrackParams.make(kmax=4)):
        got, want = _both(vb, "specials", x32, params, ext, track, N0, H0, F)
        # (statuses, VBX_FRAME_ERR_NAN where the f64 call reports it, are compared above; that the specials ARRIVED shows in the RMS column)
        rms = got[0][:, -1]
        assert np.isnan(rms[22]) and np.isnan(rms[23]) and np.isinf(rms[16]) and np.isinf(rms[17]) and 1e36 < rms[28] < np.inf and np.isfinite(rms[4]) and np.isfinite(rms[10])
    # a frame of nothing but subnormals: every sample would vanish if the conversion flushed
    x32 = np.full((F - 1) * H0 + N0, 1e-40, dtype=np.float32)
    x32[::7] = -3e-41
    got, want = _both(vb, "subnormal frames", x32, params, ext, None, N0, H0, F)
    assert np.all(got[0][:, -1] > 0.0)                          # the RMS column saw them
    # ... tracked, so that the float-max peak kernels run on them (with the RMS column: the peak branch of the RMS kernel; without
    # it: the peak kernel): a frame's peak is a subnormal float, widened -- a flushing max would give 0
    tiny = np.float64(np.float32(1e-40))
    track = pkg.PitchTrackParams.make(kmax=4)
    for e in (ext, None):
        got, want = _both(vb, "subnormal frames, tracked", x32, params, e, track, N0, H0, F)
        assert np.array_equal(_u64(got[2][2]), _u64(np.full(F, tiny))), got[2][2][:4]
    # frames of nothing but NaNs (30 and 31 whole, their neighbours in part) among ordinary ones: the peak ignores NaNs as the
    # f64 kernel does, and the statuses are the f64 call's (both compared in _both)
    x32 = synth32[:(F - 1) * H0 + N0].copy()
    x32[30 * H0:31 * H0 + N0] = np.nan
    for e in (ext, None):
        for tk in (None, track):
            got, want = _both(vb, "all-NaN frames", x32, params, e, tk, N0, H0, F)
            if e is not None:
                assert np.isnan(got[0][30, -1]) and np.isnan(got[0][31, -1])


# ---- 4. layouts --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [480, 481])
@pytest.mark.parametrize("residue", [0, 4, 8, 12])
def test_layouts_fenced(vb, pkg, synth32, stride, residue):
    F, N = 40, N0
    x32 = synth32[1000:1000 + (F - 1) * stride + N]            # the last frame ends on the buffer's last element
    params = _params(pkg)
    ext = pkg.AnalysisExt.make(0.25, rms=True)
    track = pkg.PitchTrackParams.make(kmax=4)
    width = _width(vb, params, ext)
    ld = width + (width & 1) + 6
    want_rec, want_st, want_lists, _ = _call(vb, vb.analyze_frames_ex_f32in, np.ascontiguousarray(x32), params, ext, track, N, stride, F)
    a = la.Arena(la.DeviceBackend(vb), f"f32in stride {stride} residue {residue}")
    a.input("x", x32, residue=residue)
    a.output("records", np.float64, F, width, ld=ld)
    a.output("status3", np.int32, 3, F)
    a.output("index", np.int32, 1, F)
    a.output("peak", np.float64, 1, F)
    a.place()
    outputs = pkg.PitchTrackOutputs(None, None, a["peak"], a["index"])
    assert vb.analyze_frames_ex_f32in(a["x"], params, ext, track, frame_len=N, stride=stride, n_frames=F, out=a["records"],
                                      record_ld=ld, status=a["status3"], outputs=outputs) is None
    out = a.finish()                                           # every fence and padding column intact
    la.assert_same_bits(a.label, "records", out["records"], want_rec)
    la.assert_no_new_nan(a.label, "records", out["records"], want_rec)
    la.assert_same_bits(a.label, "status3", out["status3"], want_st)
    la.assert_same_bits(a.label, "index", out["index"][0], want_lists[3])
    la.assert_same_bits(a.label, "peak", out["peak"][0], want_lists[2])
    # ... and the aligned dense call is the f64 call's
    x64 = x32.astype(np.float64)
    ref = _call(vb, vb.analyze_frames_ex, x64, params, ext, track, N, stride, F)
    la.assert_same_bits(a.label, "records vs f64", out["records"], ref[0])


# ---- 5. widened-first shapes ---------------------------------------------------------------------------------------------------------

WIDENED = [(1024, 512, 120), (2048, 1024, 60), (1103, 441, 120), (600, 240, 200), (400, 160, 300), (4100, 2050, 3)]


@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("N,H,F", WIDENED)
def test_widened_first_shapes(vb, pkg, synth32, N, H, F, tracked):
    x32 = synth32[:(F - 1) * H + N]
    params = _params(pkg)
    ext = pkg.AnalysisExt.make(0.0, rms=True)
    track = pkg.PitchTrackParams.make(kmax=4) if tracked else None
    vb.profile(True)
    vb.profile_reset()
    try:
        _both(vb, f"{N}/{H}", x32, params, ext, track, N, H, F)
        rep = vb.profile_report()
        assert WIDEN in rep and rep[WIDEN][1] == 1, sorted(rep)             # one widening pass, in the float call alone
    finally:
        vb.profile(False)


# ---- 7. errors and the empty batch ---------------------------------------------------------------------------------------------------

def test_errors_and_the_empty_batch(vb, pkg, synth32):
    F = 20
    x32 = np.ascontiguousarray(synth32[:(F - 1) * H0 + N0])
    params = _params(pkg)
    ext = pkg.AnalysisExt.make(0.25, rms=True)
    track = pkg.PitchTrackParams.make(kmax=4)
    width = _width(vb, params, ext)
    ld = width + (width & 1)
    fn = vb.L.vbx_analyze_frames_ex_f32in
    rec, st = vb.empty((F, ld)), vb.empty((3, F), np.int32)
    # a NULL x with frames to read
    assert fn(vb.ctx, None, F, N0, H0, C.byref(params), C.byref(ext), None, None, 0, rec.ptr, ld, st.ptr, None) == E_INVALID
    assert fn(vb.ctx, None, F, N0, H0, C.byref(params), C.byref(ext), C.byref(track), None, 0, rec.ptr, ld, st.ptr, None) == E_INVALID
    # records at 8 mod 16: rejected before anything is written
    a = la.Arena(la.DeviceBackend(vb), "records at 8 mod 16")
    a.input("x", x32)
    a.output("records", np.float64, F, ld, residue=8)
    a.output("status3", np.int32, 3, F)
    a.place()
    for tk in (None, C.byref(track)):
        assert fn(vb.ctx, a["x"], F, N0, H0, C.byref(params), C.byref(ext), tk, None, 0, a["records"], ld, a["status3"], None) == E_INVALID
    out = a.finish()
    assert la.unwritten(out["records"]).shape[0] == out["records"].size and la.unwritten(out["status3"]).shape[0] == out["status3"].size
    # what the f64 call rejects: a bad ratio, a frame that does not exist, an odd record_ld
    bad = pkg.AnalysisExt.make(-1.0)
    xd = vb.to_device(x32, np.float32)
    assert fn(vb.ctx, xd.ptr, F, N0, H0, C.byref(params), C.byref(bad), None, None, 0, rec.ptr, ld, st.ptr, None) == E_INVALID
    assert fn(vb.ctx, xd.ptr, F, 0, H0, C.byref(params), None, None, None, 0, rec.ptr, ld, st.ptr, None) == E_INVALID
    assert fn(vb.ctx, xd.ptr, F, N0, H0, C.byref(params), C.byref(ext), None, None, 0, rec.ptr, ld + 1, st.ptr, None) == E_INVALID
    # the empty batch succeeds (a NULL x is fine there), and a tracked one leaves an empty path
    assert fn(vb.ctx, None, 0, N0, H0, C.byref(params), C.byref(ext), None, None, 0, None, ld, None, None) == 0
    assert fn(vb.ctx, None, 0, N0, H0, C.byref(params), C.byref(ext), C.byref(track), None, 0, None, ld, None, None) == 0
    empty = _probes(vb)
    assert vb.L.vbx_analyze_frames_ex_f64(vb.ctx, None, 0, N0, H0, C.byref(params), C.byref(ext), C.byref(track), None, 0, None, ld, None, None) == 0
    assert empty == _probes(vb) and empty[3] == 0, (empty, _probes(vb))
    # the context is usable afterwards
    got = _call(vb, vb.analyze_frames_ex_f32in, xd, params, ext, track, N0, H0, F)
    want = _call(vb, vb.analyze_frames_ex, x32.astype(np.float64), params, ext, track, N0, H0, F)
    _assert_same("after the errors", got, want)
    for d in (rec, st, xd):
        d.free()
