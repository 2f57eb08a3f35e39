"""The fused frame loop's 1200-point kernel picks its instance at the launch: the launch-specialised one (SP_SPEC_*, vbx_spectral.hpp:
three wavefronts, full f64 or 16-bit PCM frames, the lag window's reciprocal table present, list in the lanes, at most sixteen
MFCC coefficients with the tail deferred; the analysis window's presence is NOT one of its conditions) or the generic one.  Both must write the same records, whatever the frames' alignment.

67 frames of 1200 / 480 of the synthetic recording (more than 64: the frames are dealt across the XCDs).  For LPC on / off x MFCC
on / off, MFCC with 13 and with 20 coefficients (both tails; 20 keeps the generic instance) and the tracked call at kmax 1 and 4:
  * f64 samples at a 16-byte-aligned base -- the reference of everything below;
  * the same samples at a base of 8 mod 16;
  * frames 481 samples apart (the alignment alternates frame by frame) against the same frames copied densely to an aligned base;
  * 16-bit PCM against its widened copy (vbx_pcm16_to_f64);
  * every one of those again on a context created with VBX_SPECTRAL_SPEC=0, i.e. through the generic instance.
Records, statuses and, for the tracked call, lists, counts, peaks and path indices: bit for bit.  vbx_internal_last_analyze_spec
says which instance launch_analyze launched: 1 (f64) / 2 (PCM) where the launch qualifies, 0 with 20 coefficients, with the switch off, and at 1024 / 512.

Needs a real MI355X: run with `-m gpu`.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR, N, HOP, F = 48000.0, 1200, 480, 67
# (id, lpc_order, mfcc coefficients, tracked kmax or None, the instance the f64 launch must take)
CASES = [("lpc-mfcc13", 12, 13, None, 1), ("lpc", 12, 0, None, 1), ("mfcc13", 0, 13, None, 1), ("pitch-only", 0, 0, None, 1),
         ("lpc-mfcc20", 12, 20, None, 0), ("tracked-k1", 12, 13, 1, 1), ("tracked-k4", 12, 13, 4, 1)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, ref, what):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        bad = _bits(g) != _bits(r)
        cols = sorted(set(np.nonzero(bad.reshape(bad.shape[0], -1))[1].tolist())) if bad.ndim else []
        assert not bad.any(), "%s: output %d differs in %d entries, columns %s" % (what, k, int(np.count_nonzero(bad)), cols)


@pytest.fixture(scope="module")
def audio(vb):
    """the recording (long enough for 67 frames 481 apart), its 16-bit quantisation and that one widened on the device"""
    total = (F - 1) * (HOP + 1) + N
    x = vb.synth_speech(total, sample_offset=5 * 48000 + 321)
    host = x.numpy()
    x.free()
    pcm = np.clip(np.rint(host * 20000.0), -32767, 32767).astype(np.int16)
    wide = vb.pcm16_to_f64(pcm)
    wide_host = wide.numpy()
    wide.free()
    return host, pcm, wide_host


@pytest.fixture(scope="module")
def vb_generic(pkg):
    """a second context, created with the switch off (the library reads it once, when a context is created)"""
    old = os.environ.get("VBX_SPECTRAL_SPEC")
    os.environ["VBX_SPECTRAL_SPEC"] = "0"
    try:
        ctx = pkg.VoxBox(0)
    finally:
        if old is None:
            del os.environ["VBX_SPECTRAL_SPEC"]
        else:
            os.environ["VBX_SPECTRAL_SPEC"] = old
    yield ctx
    ctx.close()


def _run(vb, pkg, params, kmax, x, stride, pcm=False):
    """-> (outputs, the instance that was launched); x: a device address or buffer of the context vb"""
    track = None if kmax is None else pkg.PitchTrackParams.make(kmax=kmax, time_step=0.01)
    if track is None:
        fn = vb.analyze_frames_pcm16 if pcm else vb.analyze_frames
        out = fn(x, params, frame_len=N, stride=stride, n_frames=F)
    else:
        fn = vb.analyze_frames_tracked_pcm16 if pcm else vb.analyze_frames_tracked
        out = fn(x, params, track, frame_len=N, stride=stride, n_frames=F, lists=True)
    width = max(c0 + w for c0, w in params.columns().values())      # (a record row may end in a padding column nobody writes)
    out = (out[0][:, :width],) + tuple(out[1:])
    return out, int(vb.L.vbx_internal_last_analyze_spec(vb.ctx))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_launch_variant_writes_the_aligned_f64_records(vb, vb_generic, pkg, audio, case):
    _, lpc, mfcc, kmax, want = case
    host, pcm, wide = audio
    params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=lpc, formant_order=12,
                                     mfcc=(mfcc, 100.0, 8000.0) if mfcc else None)
    bufs = []

    def dev(ctx, a, dtype=np.float64):
        bufs.append(ctx.to_device(a, dtype))
        return bufs[-1]

    try:
        aligned = dev(vb, host)
        assert aligned.ptr % 16 == 0
        ref, spec = _run(vb, pkg, params, kmax, aligned, HOP)
        assert spec == want
        dense_frames = np.stack([host[t * (HOP + 1):t * (HOP + 1) + N] for t in range(F)]).reshape(-1)
        ref_odd, _ = _run(vb, pkg, params, kmax, dev(vb, dense_frames), N)
        ref_wide, _ = _run(vb, pkg, params, kmax, dev(vb, wide), HOP)
        for ctx, on in ((vb, True), (vb_generic, False)):
            exp_f64, exp_pcm = (want, 2 if want else 0) if on else (0, 0)
            al = aligned if on else dev(ctx, host)
            got, spec = _run(ctx, pkg, params, kmax, al, HOP)
            assert spec == exp_f64
            _same(got, ref, "aligned, spec %s" % on)
            shifted = dev(ctx, np.concatenate(([0.0], host)))
            got, spec = _run(ctx, pkg, params, kmax, shifted.ptr + 8, HOP)
            assert spec == exp_f64
            _same(got, ref, "base 8 mod 16, spec %s" % on)
            got, spec = _run(ctx, pkg, params, kmax, al, HOP + 1)
            assert spec == exp_f64
            _same(got, ref_odd, "stride 481, spec %s" % on)
            got, spec = _run(ctx, pkg, params, kmax, dev(ctx, pcm, np.int16), HOP, pcm=True)
            assert spec == exp_pcm
            _same(got, ref_wide, "16-bit PCM, spec %s" % on)
            odd_pcm = dev(ctx, np.concatenate(([0], pcm)), np.int16)   # a PCM base of 2 mod 4: the two-load arm
            got, spec = _run(ctx, pkg, params, kmax, odd_pcm.ptr + 2, HOP, pcm=True)
            assert spec == exp_pcm
            _same(got, ref_wide, "16-bit PCM at 2 mod 4, spec %s" % on)
    finally:
        for b in bufs:
            b.free()


def test_other_shapes_keep_the_generic_instance(vb, pkg):
    params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=12, mfcc=(13, 100.0, 8000.0))
    for n, hop in ((1024, 512), (1103, 441)):
        x = vb.synth_speech((F - 1) * hop + n)
        try:
            vb.analyze_frames(x, params, frame_len=n, stride=hop, n_frames=F)
            assert int(vb.L.vbx_internal_last_analyze_spec(vb.ctx)) == 0
        finally:
            x.free()
