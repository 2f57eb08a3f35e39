"""The choice is what ran: after a real call of the fused frame loop, the probes of what launch_analyze did (vbx_internal_last_analyze_spec,
_last_spectral_split, _last_batching, and _last_pitch_form after vbx_pitch_f64) equal what vbx_internal_analyze_choice -- choose_analyze
asked without a GPU -- answers for that shape, and the records are the oracle's within the tolerances of tests/test_gpu_analyze.py.

67 frames; pitch + LPC(12) + 13 MFCCs, no formants: the columns the fused kernel itself leaves, and no other host loop of the call
counts batches (vbx_internal_last_batching keeps the loop with the most launches).  A context of its own per shape: a shape that no
instance serves (4097 samples: the long-frame kernels) makes no launch, and the probes then say what a fresh context says."""
import numpy as np
import pytest

from analyze_choice_cases import SP_ANALYZE_INTERP_SPLIT, SP_ANALYZE_SPLIT, probe_kw
from analyze_reference import oracle_records
from conftest import rel_close

pytestmark = pytest.mark.gpu

SR, F, ORACLE_FRAMES = 48000.0, 67, 24
PITCH, MFCC = (0.2, 75.0, 600.0), (13, 100.0, 8000.0)
SHAPES = [(1200, 480, "f64"), (1200, 480, "pcm16"), (1200, 480, "f32"), (1103, 441, "f64"), (1024, 512, "f64"), (2048, 1024, "f64"),
          (4096, 2048, "f64"), (4097, 2048, "f64")]
KIND = {"f64": 0, "pcm16": 1, "f32": 2}
PLAN_NC = {1: 1200, 2: 1024, 3: 2048, 4: 4096}


def _expected_choice(pkg, n, kind, kmax, fused_columns):
    """The launch the frame loop (fused_columns) or vbx_pitch_f64 makes for the shape, as launch_spectral describes it: MFCC's log10 + DCT
    deferred in the 1200-point plan, bins interpolated where the frame does not divide the transform, and -- where the choice says the
    shape can split -- scratch for max(1024, F) frames of the bytes per frame the choice itself names."""
    kw = dict(n=n, kind=KIND[kind], kmax=kmax)
    if fused_columns:
        bins, bad = pkg.mfcc_bins(n, MFCC[0], MFCC[1], MFCC[2], SR)
        assert not bad
        kw.update(lpc=1, coeffs=MFCC[0], nb=int(bins[-1] - bins[0]), b_lo=int(bins[0]))
        first = probe_kw(pkg, **kw)
        if first is None or first["plan"] == 0 or (2 * PLAN_NC[first["plan"]]) % n != 0:
            kw["interp"] = 1
        c = probe_kw(pkg, **kw)
        kw["defer"] = int(c["plan"] == 1)
    c = probe_kw(pkg, **kw)
    if c["split_row_bytes"]:
        c = probe_kw(pkg, scratch=max(1024, F) * c["split_row_bytes"] + 64, **kw)
    return c


@pytest.fixture(scope="module")
def audio(pkg):
    import importlib
    import __graft_entry__ as g
    synth = importlib.import_module(g.PKG_NAME + ".synth")                    # (the host form of vbx_synth_speech_f64)
    return synth.synth_speech((F - 1) * 2048 + 4097, sample_offset=2 * 48000)


@pytest.fixture(scope="module")
def references(oracle, audio):
    """shape, kind -> the oracle's records of the first ORACLE_FRAMES frames, computed once"""
    memo = {}

    def get(n, hop, kind):
        if (n, hop, kind) not in memo:
            x = _samples(audio, kind)[1]
            memo[(n, hop, kind)] = oracle_records(oracle, x, n, hop, range(ORACLE_FRAMES), SR, PITCH, 12, 0, None, MFCC, None)
        return memo[(n, hop, kind)]
    return get


def _samples(audio, kind):
    """-> (what the call reads, the f64 samples it stands for)"""
    if kind == "pcm16":
        pcm = np.clip(np.rint(audio * 32767.0), -32767, 32767).astype(np.int16)
        return pcm, pcm.astype(np.float64) / 32767.0
    if kind == "f32":
        return audio.astype(np.float32), audio.astype(np.float32).astype(np.float64)
    return audio, audio


def _check_records(rec, st, ref, top_of_list=None):
    orec, ost, _, _ = ref
    sub = ORACLE_FRAMES
    assert np.array_equal(st[:, :sub], ost)
    pitch = rec[:sub, 0:2] if top_of_list is None else top_of_list[:sub]
    assert np.all((orec[:, 0] == 0.0) == (pitch[:, 0] == 0.0)), "voiced / unvoiced decision differs"
    assert np.all(np.abs(pitch[:, 0] - orec[:, 0]) <= 1e-4 * np.abs(orec[:, 0]))
    assert np.all(np.abs(pitch[:, 1] - orec[:, 1]) <= 1e-4)
    for t in range(sub):
        assert np.all(rel_close(rec[t, 2:15], orec[t, 2:15])), t          # MFCC
        assert np.all(rel_close(rec[t, 15:28], orec[t, 15:28])), t        # LPC


@pytest.mark.parametrize("n,hop,kind", SHAPES, ids=["%d_%d_%s" % s for s in SHAPES])
def test_the_probes_say_what_the_choice_says(pkg, audio, references, n, hop, kind):
    params = pkg.AnalysisParams.make(SR, pitch=PITCH, lpc_order=12, formant_order=0, mfcc=MFCC)
    assert params.columns() == {"pitch": (0, 2), "mfcc": (2, 13), "lpc": (15, 13)}
    track = pkg.PitchTrackParams.make(kmax=4, time_step=0.01)
    x_host, _ = _samples(audio, kind)
    ref = references(n, hop, kind)
    ctx = pkg.VoxBox(0)
    try:
        x = ctx.to_device(x_host, x_host.dtype)

        def probes():
            return (int(ctx.L.vbx_internal_last_analyze_spec(ctx.ctx)), int(ctx.L.vbx_internal_last_spectral_split(ctx.ctx)), ctx.last_batching())

        def said(c):
            if c["refused"]:
                return (0, 0, None)
            split = c["mode"] in (SP_ANALYZE_SPLIT, SP_ANALYZE_INTERP_SPLIT)
            return (c["spec"], int(split), (-(-F // c["per_launch"]), c["per_launch"]) if split else (0, 0))

        def agree(c, what):
            got, want = probes(), said(c)
            print(what, n, hop, kind, "probes", got, "choice", want, {k: c[k] for k in ("refused", "family", "plan", "mode", "waves", "spec", "list", "lds")})
            assert got[:2] == want[:2], what
            assert want[2] is None or got[2] == want[2], what      # (a shape no instance serves: the long-frame loops count their own batches)

        # plain: the records' top candidate (kmax = 1)
        if kind == "pcm16":
            rec, st = ctx.analyze_frames_pcm16(x, params, frame_len=n, stride=hop, n_frames=F)
        elif kind == "f32":
            rec, st = ctx.analyze_frames_ex_f32in(x, params, frame_len=n, stride=hop, n_frames=F)[:2]
        else:
            rec, st = ctx.analyze_frames(x, params, frame_len=n, stride=hop, n_frames=F)
        agree(_expected_choice(pkg, n, kind, 1, True), "plain")
        _check_records(rec, st, ref)
        # tracked at kmax = 4: the call's own lists (their best entry is the plain call's candidate), the path in columns 0-1
        if kind == "pcm16":
            out = ctx.analyze_frames_tracked_pcm16(x, params, track, frame_len=n, stride=hop, n_frames=F, lists=True)
        elif kind == "f32":
            out = ctx.analyze_frames_ex_f32in(x, params, track=track, frame_len=n, stride=hop, n_frames=F, lists=True)
        else:
            out = ctx.analyze_frames_tracked(x, params, track, frame_len=n, stride=hop, n_frames=F, lists=True)
        agree(_expected_choice(pkg, n, kind, 4, True), "tracked")
        _check_records(out[0], out[1], ref, top_of_list=out[2][:, 0, :])
        # vbx_pitch_f64 (f64 samples): the list form comes from the same choice
        if kind == "f64":
            c = _expected_choice(pkg, n, kind, 4, False)
            han = ctx.window(pkg.WINDOW_HANNING, n)
            ctx.pitch(x, SR, PITCH[0], PITCH[1], PITCH[2], kmax=4, frame_len=n, stride=hop, n_frames=F, window=han)
            form = int(ctx.L.vbx_internal_last_pitch_form(ctx.ctx))
            print("pitch", n, hop, "form", form, "choice", {k: c[k] for k in ("refused", "plan", "list", "mode")})
            assert form == (100 if c["refused"] else 100 * (3 + c["plan"]) + c["list"])
            if not c["refused"]:
                assert probes() == said(c)
        x.free()
    finally:
        ctx.close()
