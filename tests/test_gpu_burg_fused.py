"""Burg's lag sums from the analyze kernel's own wavefronts (analyze_kernel<.., BURG>, vbx_spectral_1200.hpp): large calls of full
1200-sample f64 / PCM frames with find_formants at order 12 launch the fused instances and no burg_lags kernel, and the formant chain
runs behind the analyze kernel launch by launch (vbx_api_frames.hip, find_formants_ranges_*).  The records must not notice.

Every case runs the same call on two contexts -- one created with VBX_BURG_FUSED=0 (burg_lags_kernel beside the analyze kernel, as
before), one with VBX_BURG_FUSED_MIN_FRAMES=1 and VBX_ANALYZE_LAUNCH_FRAMES=1000 (the fused path from the first frame, a launch
every 1000 frames) -- and compares every record column, status3 and last_burg_direct_count bit for bit, and the profile report's
kernel names: the same, but for burg_lags, which only the first context launches.

All shapes 1200 / 480.  Frame counts 1, 63, 64, 65 (the scratch tile's edge), 999, 1000, 1001 (the launch cut) and 3137 (four
launches, the last one short); f64 and 16-bit PCM; a base 8 bytes (PCM: 2 bytes) off alignment and frames 481 apart; the synthetic
recording from its third second on (its fifth is noise only: frames 100..199), with a pure tone, a silent frame, a frame of -0.0 and
one NaN sample put in (the NaN in f64 only; the tone and the silence leave the one-pass guard for the direct list: asserted on the count);
one utterance, utterances of 383 frames (their cuts never coincide with a launch cut; under the lane-per-utterance scan and, forced,
under the chunked scan by ranges), and a tracked call at kmax 2.  With formant order 10 the call keeps burg_lags.

Needs a real MI355X: run with `-m gpu`.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR, N, HOP = 48000.0, 1200, 480
F_MAX = 3137
COUNTS = [1, 63, 64, 65, 999, 1000, 1001, 3137]
# frames put into the recording (by index at hop 480): a pure tone, silence, -0.0, and one NaN sample inside frame 30
TONE, SILENT, NEG_ZERO, NAN_AT = (40, 1000, 2004), (50, 1998), (20,), 30 * HOP + 601


def _ctx(pkg, env):
    """a context created under `env` (the library reads these switches once, when a context is created)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.VoxBox(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def vb_beside(pkg):
    ctx = _ctx(pkg, {"VBX_BURG_FUSED": "0"})
    ctx.profile(True)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def vb_fused(pkg):
    ctx = _ctx(pkg, {"VBX_BURG_FUSED_MIN_FRAMES": "1", "VBX_ANALYZE_LAUNCH_FRAMES": "1000"})
    ctx.profile(True)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def signal(vb):
    """(f64 samples with the special frames put in, their 16-bit quantisation -- without the NaN, which PCM cannot hold)"""
    total = (F_MAX - 1) * (HOP + 1) + N + 8
    x = vb.synth_speech(total, sample_offset=3 * 48000)
    host = x.numpy().copy()
    x.free()
    t = np.arange(N)
    for f in TONE:
        host[f * HOP:f * HOP + N] = 0.5 * np.sin(2.0 * np.pi * 220.0 * t / SR)
    for f in SILENT:
        host[f * HOP:f * HOP + N] = 0.0
    for f in NEG_ZERO:
        host[f * HOP:f * HOP + N] = -0.0
    pcm = np.clip(np.rint(host * 20000.0), -32767, 32767).astype(np.int16)
    host[NAN_AT] = np.nan
    return host, pcm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _call(ctx, pkg, x, n_frames, stride, pcm, order, seg, kmax):
    params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=order, mfcc=(13, 100.0, 8000.0))
    ctx.profile_reset()
    if kmax is not None:
        track = pkg.PitchTrackParams.make(kmax=kmax, time_step=0.01)
        fn = ctx.analyze_frames_tracked_pcm16 if pcm else ctx.analyze_frames_tracked
        out = fn(x, params, track, seg_start=seg, frame_len=N, stride=stride, n_frames=n_frames, lists=True)
    else:
        fn = ctx.analyze_frames_pcm16 if pcm else ctx.analyze_frames
        out = fn(x, params, seg_start=seg, frame_len=N, stride=stride, n_frames=n_frames)
    width = max(c0 + w for c0, w in params.columns().values())      # (a record row may end in a padding column nobody writes)
    out = (out[0][:, :width],) + tuple(out[1:])
    return out, ctx.last_burg_direct_count(), set(ctx.profile_report())


def _compare(vb_beside, vb_fused, pkg, signal, n_frames, pcm=False, stride=HOP, skew=0, order=12, seg=None, kmax=None, fused=True):
    host, pcm16 = signal
    src, dtype, size = (pcm16, np.int16, 2) if pcm else (host, np.float64, 8)
    need = (n_frames - 1) * stride + N
    src = np.concatenate((np.zeros(skew, dtype), src[:need]))
    res = []
    for ctx in (vb_beside, vb_fused):
        buf = ctx.to_device(src, dtype)
        try:
            assert buf.ptr % 16 == 0
            res.append(_call(ctx, pkg, buf.ptr + skew * size, n_frames, stride, pcm, order, seg, kmax))
        finally:
            buf.free()
    (ref, ref_direct, ref_names), (got, got_direct, got_names) = res
    assert "burg_lags" in ref_names
    assert ("burg_lags" not in got_names) == fused, sorted(got_names)
    assert got_names | {"burg_lags"} == ref_names, (sorted(got_names), sorted(ref_names))
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape, (k, g.shape, r.shape)
        bad = _bits(g) != _bits(r)
        cols = sorted(set(np.nonzero(bad.reshape(bad.shape[0], -1))[1].tolist())) if bad.ndim > 1 else []
        assert not bad.any(), "output %d differs in %d entries (rows %s ..., columns %s)" % (
            k, int(np.count_nonzero(bad)), np.nonzero(bad.reshape(bad.shape[0], -1).any(axis=1))[0][:8].tolist() if bad.ndim > 1 else "-", cols)
    assert got_direct == ref_direct
    return ref_direct


@pytest.mark.parametrize("pcm", [False, True], ids=["f64", "pcm16"])
@pytest.mark.parametrize("n_frames", COUNTS)
def test_one_utterance(vb_beside, vb_fused, pkg, signal, n_frames, pcm):
    direct = _compare(vb_beside, vb_fused, pkg, signal, n_frames, pcm=pcm)
    # the silent frame and the frame of -0.0 (no positive denominator) and the f64 tone (a singular system) always leave the one-pass
    # guard; the quantised tone carries 16-bit rounding noise and need not
    special = [f for f in SILENT + NEG_ZERO + (() if pcm else TONE) if f < n_frames]
    assert direct >= len(special), (direct, special)


@pytest.mark.parametrize("pcm", [False, True], ids=["f64", "pcm16"])
def test_base_off_alignment(vb_beside, vb_fused, pkg, signal, pcm):
    _compare(vb_beside, vb_fused, pkg, signal, 1001, pcm=pcm, skew=1)          # 8 bytes (PCM: 2 bytes) past a 16-byte boundary


@pytest.mark.parametrize("pcm", [False, True], ids=["f64", "pcm16"])
def test_frames_481_apart(vb_beside, vb_fused, pkg, signal, pcm):
    _compare(vb_beside, vb_fused, pkg, signal, 1001, pcm=pcm, stride=HOP + 1)


@pytest.mark.parametrize("chunked", [None, "1"], ids=["lane-per-utterance", "chunked-by-ranges"])
def test_utterances_of_383_frames(vb_beside, vb_fused, pkg, signal, monkeypatch, chunked):
    if chunked is not None:
        monkeypatch.setenv("VBX_TRACKER_CHUNKED", chunked)                       # (read per call, by both contexts)
    seg = np.arange(0, F_MAX, 383, dtype=np.int64)
    assert not any(int(s) % 1000 == 0 for s in seg[1:])
    _compare(vb_beside, vb_fused, pkg, signal, F_MAX, seg=seg)


def test_tracked_call_at_kmax_2(vb_beside, vb_fused, pkg, signal):
    _compare(vb_beside, vb_fused, pkg, signal, 1001, seg=np.arange(0, 1001, 383, dtype=np.int64), kmax=2)


def test_order_10_keeps_the_lag_kernel(vb_beside, vb_fused, pkg, signal):
    _compare(vb_beside, vb_fused, pkg, signal, 1001, order=10, fused=False)
