"""vbx_analyze_frames_tracked_f64 / _pcm16 on a real MI355X: the fused frame loop whose columns 0-1 hold the pitch path over the
call's own candidate lists.  Everything but the pitch columns is the plain call's, bit for bit; the contour is vbx_pitch_path_f64's
on the returned lists, bit for bit; the lists are vbx_pitch_f64's at the project's tolerances; the PCM form equals widen + f64."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import layout_arena as la
import pitch_path_model as M

pytestmark = pytest.mark.gpu

SR, P = 48000.0, 12
SHAPES = [(1200, 480), (1024, 512), (1103, 441), (2048, 1024), (4096, 2048), (256, 128), (5000, 2500)]
REPORT = {}


def _kmaxes(N):
    return (1, 3, 4, 15, 63) if N == 1200 else (1, 3, 4, 15)


@pytest.fixture(scope="module", autouse=True)
def report():
    """Prints what the list and model comparisons of this module recorded, after its last test."""
    yield
    lists = {k: v for k, v in REPORT.items() if k.startswith("lists_")}
    print("\nanalyze_tracked report:", REPORT)
    print("lists bit-identical to vbx_pitch_f64 on", sum(1 for v in lists.values() if v[3]), "of", len(lists), "cases")


@pytest.fixture(scope="module")
def audio_d(vb):
    d = vb.synth_speech(6 * 48000, sample_offset=2 * 48000)     # voiced glide + one unvoiced second
    yield d
    d.free()


def _seg(F):
    q = min(F // 4, 150)
    return np.array([0, q, q + 1, min(400, F - 10)], dtype=np.int64)              # a one-frame utterance among them


def _i64(a):
    return np.ascontiguousarray(a).view(np.int64)


def _listed(cand, count):
    """The lists with everything behind count[t] zeroed (entries no one defines)."""
    c = np.array(cand, copy=True)
    c[np.arange(c.shape[1])[None, :] >= np.asarray(count)[:, None]] = 0.0
    return c


def _tracked(vb, pkg, x, params, kmax, seg, N, H, F, pcm=False, **path_kw):
    track = pkg.PitchTrackParams.make(kmax=kmax, **path_kw)
    fn = vb.analyze_frames_tracked_pcm16 if pcm else vb.analyze_frames_tracked
    rec, st, cand, count, peak, index = fn(x, params, track, seg_start=seg, frame_len=N, stride=H, n_frames=F, lists=True)
    return rec, st, _listed(cand, count), count, peak, index


def _read_wav16(path):
    with wave.open(path, "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        return pcm.astype(np.float64) / 32767.0, float(w.getframerate())


def _golden_params(pkg, sr):
    return pkg.AnalysisParams.make(sr, mfcc=(13, 100.0, min(8000.0, 0.45 * sr)))


# ---- 1. everything but pitch is untouched ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("policy", ["EXACT", "REFERENCE"])
@pytest.mark.parametrize("N,H", SHAPES)
def test_everything_but_pitch_is_the_plain_call(vb, pkg, audio_d, N, H, policy):
    F = pkg.frame_count(6 * 48000, N, H)
    seg = _seg(F)
    params = pkg.AnalysisParams.make(SR)
    old = vb.lpc_policy
    vb.lpc_policy = getattr(pkg, "LPC_POLICY_" + policy)
    try:
        rec0, st0 = vb.analyze_frames(audio_d, params, seg_start=seg, frame_len=N, stride=H, n_frames=F)
        exact0 = vb.last_lpc_exact_count()
        for kmax in _kmaxes(N):
            rec, st, *_ = _tracked(vb, pkg, audio_d, params, kmax, seg, N, H, F)
            assert vb.last_lpc_exact_count() == exact0, (kmax, exact0)          # the LPC probe reports as after the plain call
            assert rec.shape == rec0.shape == (F, 36)
            assert np.array_equal(_i64(rec[:, 2:]), _i64(rec0[:, 2:])), (N, H, kmax, policy)
            assert np.array_equal(st, st0), (N, H, kmax, policy)
    finally:
        vb.lpc_policy = old


# ---- 2. the contour is the path of the call's own lists -----------------------------------------------------------------------------

@pytest.mark.parametrize("N,H", SHAPES)
def test_contour_is_the_path_of_the_returned_lists(vb, pkg, audio_d, N, H):
    F = pkg.frame_count(6 * 48000, N, H)
    seg = _seg(F)
    params = pkg.AnalysisParams.make(SR)
    lp_ref = vb.frame_peak(audio_d, frame_len=N, stride=H, n_frames=F)
    for kmax in _kmaxes(N):
        rec, st, cand, count, peak, index = _tracked(vb, pkg, audio_d, params, kmax, seg, N, H, F)
        assert vb.last_path_chunks_redone() >= 0
        assert np.array_equal(_i64(peak), _i64(lp_ref)), (N, kmax)              # vbx_frame_peak_f64, bit for bit
        pp = pkg.PitchPathParams.make(time_step=H / SR)
        path, idx = vb.pitch_path(cand, count, st[0], peak, seg_start=seg, params=pp)
        assert np.array_equal(index, idx), (N, kmax)
        assert np.array_equal(_i64(rec[:, 0:2]), _i64(path)), (N, kmax)
        # the same with the optional outputs NULL (context-owned lists) ...
        track = pkg.PitchTrackParams.make(kmax=kmax)
        rec_n, st_n = vb.analyze_frames_tracked(audio_d, params, track, seg_start=seg, frame_len=N, stride=H, n_frames=F)
        assert np.array_equal(_i64(rec_n), _i64(rec)) and np.array_equal(st_n, st), (N, kmax)
        # ... with an explicit time_step, and as one sequential scan per segment
        for kw in (dict(time_step=H / SR), dict(chunk_frames=F), dict(chunk_frames=F + 7)):
            r2, s2, c2, n2, p2, i2 = _tracked(vb, pkg, audio_d, params, kmax, seg, N, H, F, **kw)
            assert np.array_equal(_i64(r2), _i64(rec)) and np.array_equal(s2, st) and np.array_equal(i2, index), (N, kmax, kw)
            assert np.array_equal(_i64(c2), _i64(cand)) and np.array_equal(n2, count) and np.array_equal(_i64(p2), _i64(peak))
    # silence_threshold == 0 and no outputs: the contour of a path that ignores the peaks
    track = pkg.PitchTrackParams.make(kmax=4, silence_threshold=0.0)
    rec_s, st_s = vb.analyze_frames_tracked(audio_d, params, track, seg_start=seg, frame_len=N, stride=H, n_frames=F)
    _, _, cand, count, _, _ = _tracked(vb, pkg, audio_d, params, 4, seg, N, H, F)
    path, _ = vb.pitch_path(cand, count, st_s[0], None, seg_start=seg,
                            params=pkg.PitchPathParams.make(time_step=H / SR, silence_threshold=0.0))
    assert np.array_equal(_i64(rec_s[:, 0:2]), _i64(path))


# ---- 3. the lists are the library's lists ----------------------------------------------------------------------------------------

def _compare_lists(name, cand, count, st, ref_cand, ref_count, ref_st, ext_cand, ext_count):
    """count and status equal on EVERY frame.  Entries are compared by position at 1e-4 relative in Hz and 1e-4 in strength.  The two
    instantiations agree to ~1e-7, not bit for bit, so where adjacent strengths of vbx_pitch_f64's OWN list lie closer than 1e-6 the
    entries of that run of positions may come in any order: such a run is compared as an unordered set (each reference entry has
    a partner within the same tolerances, one to one), every other position of the frame by position.  A run that reaches the last
    kept position of a full list may continue behind the cut: it is held to the run of vbx_pitch_f64's list at kmax + 8 (ext_cand /
    ext_count) -- every returned entry has its own partner there.  Only if that run reaches the end of the longer list too is the
    frame left out of the entry comparison: at most 2 % of the frames.  Returns (frames left out, frames with a tied run, frames,
    every compared entry bit-identical)."""
    F, kmax = ref_cand.shape[0], ref_cand.shape[1]
    assert np.array_equal(count, ref_count), (name, np.nonzero(count != ref_count)[0][:8])
    assert np.array_equal(st, ref_st), name
    m = np.minimum(ref_count, kmax)
    col = np.arange(kmax)[None, :]
    listed = col < m[:, None]
    gap = np.abs(ref_cand[:, 1:, 1] - ref_cand[:, :-1, 1])
    link = (gap < 1e-6) & listed[:, 1:]                          # positions j and j + 1 belong to one run
    tied = np.zeros((F, kmax), bool)
    tied[:, 1:] |= link
    tied[:, :-1] |= link
    # a run that touches the last kept position of a list cut at kmax (count > kmax never shows here: counts are capped) -- the
    # cut may fall inside the run
    cut = (m == kmax) & tied[:, kmax - 1]
    use = listed & ~tied
    kext = ext_cand.shape[1]
    mext = np.minimum(ext_count, kext)
    left_out = np.zeros(F, bool)

    def close(a, b):
        return (np.abs(a[..., 0] - b[..., 0]) <= 1e-4 * np.abs(b[..., 0])) & (np.abs(a[..., 1] - b[..., 1]) <= 1e-4)
    ok = close(cand, ref_cand)
    rel = np.where(use, np.abs(cand[:, :, 0] - ref_cand[:, :, 0]) / np.maximum(np.abs(ref_cand[:, :, 0]), 1e-300), 0.0)
    print(f"{name}: frames {F}, with a tied run {int(np.any(tied, axis=1).sum())}, of those cut at kmax {int(cut.sum())}, "
          f"max rel Hz {np.max(rel):.3e}, max strength diff {np.max(np.where(use, np.abs(cand[:, :, 1] - ref_cand[:, :, 1]), 0.0)):.3e}")
    assert np.all(ok[use]), (name, np.argwhere(use & ~ok)[:8])
    same = bool(np.array_equal(_i64(cand[use]), _i64(ref_cand[use])))
    for t in np.nonzero(np.any(tied, axis=1))[0]:              # the tied runs, as unordered sets
        j = 0
        while j < kmax:
            if not tied[t, j]:
                j += 1
                continue
            k = j
            while k + 1 < kmax and link[t, k]:
                k += 1
            got, ref = cand[t, j:k + 1], ref_cand[t, j:k + 1]
            if cut[t] and k == kmax - 1:                        # the run may go on behind the cut: the longer list's run from j on
                e = k
                while e + 1 < mext[t] and abs(ext_cand[t, e + 1, 1] - ext_cand[t, e, 1]) < 1e-6:
                    e += 1
                if e == kext - 1 and mext[t] == kext:           # ... which is cut as well
                    left_out[t] = True
                    break
                ref = ext_cand[t, j:e + 1]
            free = list(range(len(ref)))
            for g in got:                                       # runs are a few entries long: greedy one-to-one matching decides
                hit = [q for q in free if close(g, ref[q])]
                assert hit, (name, int(t), j, k, got, ref)
                free.remove(hit[0])
            same = same and bool(np.array_equal(_i64(got), _i64(ref_cand[t, j:k + 1])))      # (against the list at the same kmax)
            j = k + 1
    print(f"{name}: left out {int(left_out.sum())}")
    assert left_out.sum() <= 0.02 * F, (name, int(left_out.sum()), F)
    return int(left_out.sum()), int(np.any(tied, axis=1).sum()), F, same


@pytest.mark.parametrize("N,H", SHAPES)
def test_lists_are_vbx_pitch_lists(vb, pkg, audio_d, N, H):
    F = pkg.frame_count(6 * 48000, N, H)
    seg = _seg(F)
    params = pkg.AnalysisParams.make(SR)
    han = vb.window(pkg.WINDOW_HANNING, N)
    for kmax in _kmaxes(N):
        _, st, cand, count, _, _ = _tracked(vb, pkg, audio_d, params, kmax, seg, N, H, F)
        rc, rn, rs = vb.pitch(audio_d, SR, 0.2, 75.0, 600.0, kmax=kmax, frame_len=N, stride=H, n_frames=F, window=han)
        ec, en, _ = vb.pitch(audio_d, SR, 0.2, 75.0, 600.0, kmax=kmax + 8, frame_len=N, stride=H, n_frames=F, window=han)
        REPORT[f"lists_{N}_{H}_k{kmax}"] = _compare_lists(f"synth {N}/{H} kmax {kmax}", cand, count, st[0], _listed(rc, rn), rn, rs,
                                                          _listed(ec, en), en)


@pytest.mark.parametrize("name,hop", [("sample-two_vowels", 512), ("down_sampled", 256)])
def test_lists_on_golden_speech(vb, pkg, golden_dir, name, hop):
    x, sr = _read_wav16(os.path.join(golden_dir, name + ".wav"))
    n, kmax = 1024, 15
    F = pkg.frame_count(x.size, n, hop)
    params = _golden_params(pkg, sr)
    han = vb.window(pkg.WINDOW_HANNING, n)
    _, st, cand, count, _, _ = _tracked(vb, pkg, x, params, kmax, None, n, hop, F)
    rc, rn, rs = vb.pitch(x, sr, params.pitch_threshold, params.pitch_fmin, params.pitch_fmax, kmax=kmax, frame_len=n, stride=hop,
                          window=han)
    ec, en, _ = vb.pitch(x, sr, params.pitch_threshold, params.pitch_fmin, params.pitch_fmax, kmax=kmax + 8, frame_len=n, stride=hop,
                         window=han)
    REPORT[f"lists_{name}"] = _compare_lists(f"{name} 1024/{hop}", cand, count, st[0], _listed(rc, rn), rn, rs, _listed(ec, en), en)


# ---- 4. golden speech against the numpy model -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["short_sample", "down_sampled", "sample-two_vowels"])
def test_golden_speech_index_matches_the_model(vb, pkg, golden_dir, name):
    x, sr = _read_wav16(os.path.join(golden_dir, name + ".wav"))
    n, hop = 1024, 256
    F = pkg.frame_count(x.size, n, hop)
    params = _golden_params(pkg, sr)
    for kmax in (4, 15):
        rec, st, cand, count, peak, index = _tracked(vb, pkg, x, params, kmax, None, n, hop, F)
        p = dict(M.DEFAULTS, time_step=hop / sr)
        tab = M.frame_table(cand, count, st[0], peak, None, p)
        st_m = M.path_states(tab, None)
        mp, mi = M.outputs(tab, st_m)
        # whatever the device chose, columns 0-1 are bitwise what its index selects
        own_p, own_i = M.outputs(tab, M.states_from_index(tab, index))
        assert np.array_equal(own_i, index) and np.array_equal(_i64(own_p), _i64(rec[:, 0:2])), (name, kmax)
        diff = np.nonzero(mi != index)[0]
        if diff.size:                                          # the model's near-tie rule: equal scores to 1e-12 (expected use: 0)
            a, b = M.path_score(tab, st_m, 0, F), M.path_score(tab, M.states_from_index(tab, index), 0, F)
            assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1.0), (name, kmax, a, b)
        REPORT[f"model_{name}_k{kmax}"] = int(diff.size)
        assert np.any(index >= 0)                              # voiced somewhere


# ---- 5. PCM --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,lpc_order", [(1200, 480, 12), (1200, 480, 0), (1103, 441, 12), (1200, 480, 10)])
def test_pcm16_equals_widen_then_f64(vb, pkg, audio_d, N, H, lpc_order):
    """(1200, 480) with lpc_order 12 / 0: the kernels read the PCM directly; (1103, 441) and order 10: the context-owned copy."""
    audio = audio_d.numpy()
    pcm = np.clip(np.rint(audio / np.max(np.abs(audio)) * 30000.0), -32768, 32767).astype(np.int16)
    pcm[7 * H + 100] = -32768                                  # |s| = 32768 needs 32 bits
    pcm[7 * H + 101] = 32767
    F = pkg.frame_count(pcm.size, N, H)
    seg = _seg(F)
    params = pkg.AnalysisParams.make(SR, lpc_order=lpc_order)
    pcm_d = vb.to_device(pcm, np.int16)
    wide = vb.empty(pcm.size)
    vb._check(vb.L.vbx_pcm16_to_f64(vb.ctx, pcm_d.ptr, pcm.size, wide.ptr))
    try:
        for kmax in (4, 15):
            want = _tracked(vb, pkg, wide, params, kmax, seg, N, H, F)
            got = _tracked(vb, pkg, pcm_d, params, kmax, seg, N, H, F, pcm=True)
            for w, g, what in zip(want, got, ("records", "status3", "cand", "count", "peak", "index")):
                assert w.shape == g.shape and w.dtype == g.dtype, what
                assert np.array_equal(w.view(np.uint8), g.view(np.uint8)), (what, N, lpc_order, kmax)
            assert got[4][7] == 32768.0 / 32767.0 and np.all(got[4][:5] <= 30000.0 / 32767.0)
            # NULL outputs: the same records
            rec_n, st_n = vb.analyze_frames_tracked_pcm16(pcm_d, params, pkg.PitchTrackParams.make(kmax=kmax), seg_start=seg,
                                                          frame_len=N, stride=H, n_frames=F)
            assert np.array_equal(_i64(rec_n), _i64(got[0])) and np.array_equal(st_n, got[1])
    finally:
        pcm_d.free(); wide.free()


@pytest.mark.parametrize("off", [0, 1, 3, 5])
def test_pcm16_frame_peak_at_every_row_alignment(vb, pkg, off):
    """The PCM peak kernel's head / 16-byte middle / tail split: views that start 2 * off bytes into the buffer, odd strides and
    lengths, against numpy."""
    rng = np.random.default_rng(17 + off)
    pcm = rng.integers(-32768, 32768, 60000).astype(np.int16)
    pcm_d = vb.to_device(pcm, np.int16)
    params = pkg.AnalysisParams.make(SR, lpc_order=0, formant_order=0, mfcc=None)
    try:
        for N, H in ((1200, 480), (1201, 333), (517, 259), (600, 7)):
            F = min(pkg.frame_count(pcm.size - off, N, H), 100)
            *_, peak, _ = _tracked(vb, pkg, pcm_d.ptr + 2 * off, params, 1, None, N, H, F, pcm=True)
            fr = np.lib.stride_tricks.sliding_window_view(pcm[off:].astype(np.int64), N)[::H][:F]
            assert np.array_equal(peak, np.max(np.abs(fr), axis=1) / 32767.0), (off, N, H)
    finally:
        pcm_d.free()


# ---- 6. one pass ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pcm", [False, True])
def test_one_pass_over_the_samples(pkg, pcm):
    N, H, F = 1200, 480, 400
    ctx = pkg.VoxBox(0)
    try:
        x = ctx.synth_speech((F - 1) * H + N, sample_offset=2 * 48000)
        if pcm:
            s = np.clip(np.rint(x.numpy() * 20000.0), -32768, 32767).astype(np.int16)
            x.free()
            x = ctx.to_device(s, np.int16)
        params = pkg.AnalysisParams.make(SR)
        track = pkg.PitchTrackParams.make(kmax=15)
        fn = ctx.analyze_frames_tracked_pcm16 if pcm else ctx.analyze_frames_tracked
        fn(x, params, track, frame_len=N, stride=H, n_frames=F)                  # tables, workspaces
        ctx.profile_reset(); ctx.profile(True)
        calls = 3
        for _ in range(calls):
            fn(x, params, track, frame_len=N, stride=H, n_frames=F, lists=True)
        rep = ctx.profile_report()
        streams = ctx.profile_streams()
        ctx.profile(False)
        x.free()
    finally:
        ctx.close()
    peak = "frame_peak_pcm16" if pcm else "frame_peak"
    for name in ("analyze", peak, "pitch_path_spec", "pitch_path_write"):
        assert name in rep and rep[name][1] == calls, (name, rep)                # one fused launch set per call
    assert "pitch" not in rep, sorted(rep)                                        # no pitch-only kernel
    assert "pcm16" not in rep and "frame_peak" + ("" if pcm else "_pcm16") not in rep, sorted(rep)     # nothing widens
    assert streams["analyze"] == 0 and streams["pitch_path_spec"] == 0 and streams[peak] == 1, streams


def test_no_peak_kernel_when_the_path_does_not_need_one(pkg):
    N, H, F = 1200, 480, 200
    ctx = pkg.VoxBox(0)
    try:
        x = ctx.synth_speech((F - 1) * H + N, sample_offset=2 * 48000)
        params = pkg.AnalysisParams.make(SR)
        ctx.profile_reset(); ctx.profile(True)
        ctx.analyze_frames_tracked(x, params, pkg.PitchTrackParams.make(kmax=4, silence_threshold=0.0), frame_len=N, stride=H, n_frames=F)
        rep = ctx.profile_report()
        ctx.profile(False)
        x.free()
    finally:
        ctx.close()
    assert "analyze" in rep and "pitch_path_spec" in rep
    assert not any(n.startswith("frame_peak") for n in rep) and "pitch_path_peak" not in rep, sorted(rep)


# ---- 7. misuse -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pcm", [False, True])
def test_rejected_calls_write_nothing_and_leave_the_context_usable(vb, pkg, audio_d, pcm):
    N, H, F, kmax = 1200, 480, 64, 4
    if pcm:
        s = np.clip(np.rint(audio_d.numpy()[:(F - 1) * H + N] * 20000.0), -32768, 32767).astype(np.int16)
        x = vb.to_device(s, np.int16)
        fn = vb.L.vbx_analyze_frames_tracked_pcm16
    else:
        x = vb.to_device(audio_d.numpy()[:(F - 1) * H + N])
        fn = vb.L.vbx_analyze_frames_tracked_f64
    params = pkg.AnalysisParams.make(SR)
    REC = int(vb.L.vbx_record_doubles(C.byref(params)))
    canary = {"records": np.full((F, REC), np.nan).view(np.uint64), "status3": np.full((3, F), 0x5AFEC0DE, np.uint32),
              "cand": np.full((F, 63, 2), np.nan).view(np.uint64), "count": np.full(F, 0x5AFEC0DE, np.uint32),
              "peak": np.full(F, np.nan).view(np.uint64), "index": np.full(F, 0x5AFEC0DE, np.uint32)}
    for a in ("records", "cand", "peak"):
        canary[a][...] = la.CANARY_F64
    dev = {k: vb.to_device(v) for k, v in canary.items()}
    outs = pkg.PitchTrackOutputs(dev["cand"].ptr, dev["count"].ptr, dev["peak"].ptr, dev["index"].ptr)
    good_seg = np.array([0, 10, 11], np.int64)

    def call(x_ptr=x.ptr, n=F, n_len=N, hop=H, p=params, track="default", k=kmax, seg=good_seg, rec=dev["records"].ptr, ld=REC,
             path_kw=None):
        t = pkg.PitchTrackParams.make(kmax=k, **(path_kw or {})) if track == "default" else track
        return fn(vb.ctx, x_ptr, n, n_len, hop, None if p is None else C.byref(p), None if t is None else C.byref(t),
                  None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size, rec, ld, dev["status3"].ptr, C.byref(outs))

    def variant(**kw):
        q = pkg.AnalysisParams.make(SR)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    bad = [dict(k=0), dict(k=64), dict(k=1 << 40), dict(track=None)]
    for field in ("voicing_threshold", "silence_threshold", "octave_cost", "octave_jump_cost", "voiced_unvoiced_cost", "ceiling_hz",
                  "time_step"):
        for v in (-0.1, float("nan"), float("inf")):
            bad.append(dict(path_kw={field: v}))
    bad.append(dict(path_kw=dict(ceiling_hz=0.0)))
    # what the plain call rejects
    bad += [dict(p=None), dict(ld=REC - 1), dict(ld=REC + 1), dict(ld=REC - 2), dict(rec=dev["records"].ptr + 8), dict(rec=None),
            dict(x_ptr=None), dict(n_len=0), dict(hop=0), dict(n_len=(1 << 26) + 1), dict(n=1 << 31),
            dict(p=variant(n_est=0)), dict(p=variant(n_est=7)), dict(p=variant(mfcc_coeffs=65)), dict(p=variant(formant_order=63)),
            dict(p=variant(lpc_order=63)), dict(p=variant(lpc_order=1200))]
    for s in ([1, 5], [0, 9, 5], [0, F + 1]):
        bad.append(dict(seg=np.array(s, np.int64)))
    for b in bad:
        assert call(**b) == -1, b                              # VBX_E_INVALID
        assert vb.L.vbx_last_error(vb.ctx)
    vb.sync()
    for k, d in dev.items():                                   # nothing was written
        assert np.array_equal(d.numpy().view(np.uint8), np.ascontiguousarray(canary[k]).view(np.uint8)), k
    # time_step == 0 is NOT rejected here, an empty batch succeeds, and the next valid call is right
    assert call(n=0, seg=None) == 0 and vb.last_path_chunks_redone() == 0
    assert call(path_kw=dict(time_step=0.0)) == 0
    rec = dev["records"].numpy().view(np.float64)
    want = _tracked(vb, pkg, x, params, kmax, good_seg, N, H, F, pcm=pcm)
    assert np.array_equal(_i64(rec), _i64(want[0]))
    assert np.array_equal(dev["index"].numpy().view(np.int32), want[5])
    assert np.array_equal(dev["status3"].numpy().view(np.int32), want[1])
    # the Python layer refuses the argument combinations that would drop the lists
    track = pkg.PitchTrackParams.make(kmax=kmax)
    meth = vb.analyze_frames_tracked_pcm16 if pcm else vb.analyze_frames_tracked
    for kw in (dict(out=dev["records"], record_ld=REC), dict(outputs=outs)):
        with pytest.raises(ValueError):
            meth(x, params, track, frame_len=N, stride=H, n_frames=F, lists=True, **kw)
    for d in list(dev.values()) + [x]:
        d.free()


# ---- 8. state after the call -----------------------------------------------------------------------------------------------------

def test_stitch_after_a_tracked_call_is_the_plain_stitch(vb, pkg):
    N, H = 1200, 480
    F, cut, warm = 3000, 1500, 1                               # a warm-up too short to forget: the stitch has rows to redo
    audio = vb.synth_speech((F - 1) * H + N, sample_offset=11 * 48000)
    params = pkg.AnalysisParams.make(SR)
    REC = int(vb.L.vbx_record_doubles(C.byref(params)))
    whole, _ = vb.analyze_frames(audio, params, frame_len=N, stride=H, n_frames=F)
    a = vb.empty((cut, REC))
    vb.analyze_frames(audio, params, frame_len=N, stride=H, n_frames=cut, out=a, record_ld=REC)
    state = a.ptr + ((cut - 1) * REC + 2) * 8
    first = cut - warm
    n = F - first
    changed = vb.empty(1, np.int32)
    after = {}
    for how in ("plain", "tracked"):
        b = vb.empty((n, REC))
        if how == "plain":
            vb.analyze_frames(audio.ptr + first * H * 8, params, frame_len=N, stride=H, n_frames=n, out=b, record_ld=REC)
        else:
            vb.analyze_frames_tracked(audio.ptr + first * H * 8, params, pkg.PitchTrackParams.make(kmax=4), frame_len=N, stride=H,
                                      n_frames=n, out=b, record_ld=REC)
            assert vb.last_path_chunks_redone() >= 0
        before = b.numpy()
        vb.track_stitch(b.ptr + 2 * 8, n, REC, warm, n, state, changed)
        after[how] = (before, b.numpy(), int(changed.numpy()[0]))
        b.free()
    (b0, a0, n0), (b1, a1, n1) = after["plain"], after["tracked"]
    assert n0 == n1 and n0 > 0
    assert np.array_equal(_i64(b0[:, 2:]), _i64(b1[:, 2:])) and np.array_equal(_i64(a0[:, 2:]), _i64(a1[:, 2:]))
    assert np.array_equal(_i64(a1[warm:, 2:10]), _i64(whole[cut:, 2:10]))       # the single scan's rows
    assert np.array_equal(_i64(a1[:, 0:2]), _i64(b1[:, 0:2]))                   # the stitch leaves the contour alone
    for d in (a, changed, audio):
        d.free()


# ---- 9. layouts ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,pcm", [(1200, 480, False), (1024, 512, False), (1200, 480, True)])
def test_odd_bases_and_padded_records(vb, pkg, audio_d, N, H, pcm):
    """x at 8 mod 16 (PCM: 2 mod 16), records padded to rec + 6 doubles, the lists / counts / peaks / indices at 8 mod 16, status3 at
    4 mod 16: bit-equal to the aligned dense call, fences and padding intact."""
    F, kmax = 37, 4
    sig = audio_d.numpy()[48000:48000 + (F - 1) * H + N]
    if pcm:
        sig = np.clip(np.rint(sig * 20000.0), -32768, 32767).astype(np.int16)
    params = pkg.AnalysisParams.make(SR)
    REC = int(vb.L.vbx_record_doubles(C.byref(params)))
    ld = REC + 6
    seg = np.array([0, 9, 10], np.int64)
    sig_d = vb.to_device(sig)
    want = _tracked(vb, pkg, sig_d, params, kmax, seg, N, H, F, pcm=pcm)
    sig_d.free()
    a = la.Arena(la.DeviceBackend(vb), f"analyze_tracked {N}/{H} pcm={pcm}")
    a.input("x", sig, residue=2 if pcm else 8)
    a.output("records", np.float64, F, REC, ld=ld, residue=0)
    a.output("status3", np.int32, 3, F, residue=4)
    a.output("cand", np.float64, F, 2 * kmax, residue=8)
    a.output("count", np.int32, F, 1, residue=8)
    a.output("peak", np.float64, F, 1, residue=8)
    a.output("index", np.int32, F, 1, residue=8)
    a.place()
    outs = pkg.PitchTrackOutputs(a["cand"], a["count"], a["peak"], a["index"])
    track = pkg.PitchTrackParams.make(kmax=kmax)
    fn = vb.L.vbx_analyze_frames_tracked_pcm16 if pcm else vb.L.vbx_analyze_frames_tracked_f64
    rc = fn(vb.ctx, a["x"], F, N, H, C.byref(params), C.byref(track), seg.ctypes.data, seg.size, a["records"], ld, a["status3"],
            C.byref(outs))
    assert rc == 0, vb.L.vbx_last_error(vb.ctx)
    got = a.finish()                                           # fences, padding columns and the input untouched
    label = a.label
    la.assert_written(label, "records", got["records"])
    la.assert_same_bits(label, "records", got["records"], want[0])
    la.assert_same_bits(label, "status3", got["status3"], want[1])
    count = got["count"][:, 0]
    la.assert_same_bits(label, "count", count, want[3])
    la.assert_same_bits(label, "cand", _listed(got["cand"].reshape(F, kmax, 2), count), want[2])
    la.assert_same_bits(label, "peak", got["peak"][:, 0], want[4])
    la.assert_same_bits(label, "index", got["index"][:, 0], want[5])
