"""vbx_pitch_path_f64 / vbx_frame_peak_f64 on the device: hand-built candidate lists with known answers, the numpy model
(tests/pitch_path_model.py) on random lists and on the lists vbx_pitch_f64 produces from real and synthetic speech, and the
chunked scan against the sequential one, bit for bit."""
import ctypes as C
import os
import warnings
import wave

import numpy as np
import pytest

import pitch_path_model as M

pytestmark = pytest.mark.gpu

REPORT = {}


def _params(pkg, **kw):
    return pkg.PitchPathParams.make(**kw)


def _run(vb, pkg, cand, count, status=None, local_peak=None, seg_start=None, **kw):
    return vb.pitch_path(cand, count, status, local_peak, seg_start=seg_start, params=_params(pkg, **kw))


def _model(cand, count, status=None, local_peak=None, seg_start=None, **kw):
    p = dict(M.DEFAULTS, **{k: v for k, v in kw.items() if k != "chunk_frames"})
    return M.pitch_path(cand, count, status, local_peak, seg_start, p)


def _check_against_model(cand, count, status, local_peak, seg_start, got, name, **kw):
    """out_index identical on every frame and out_path bitwise the selected entry or u_t; a frame may differ only inside a near
    tie of the model's scores (device log2 may be an ulp from numpy's).  Returns the number of such frames."""
    path, index = got
    p = dict(M.DEFAULTS, **{k: v for k, v in kw.items() if k != "chunk_frames"})
    tab = M.frame_table(cand, count, status, local_peak, seg_start, p)
    st_m = M.path_states(tab, seg_start)
    mp, mi = M.outputs(tab, st_m)
    # whatever the device chose, its out_path is bitwise what its out_index selects
    own_p, own_i = M.outputs(tab, M.states_from_index(tab, index))
    assert np.array_equal(own_i, index)
    assert np.array_equal(own_p.view(np.int64), path.view(np.int64)), name
    diff = np.nonzero(mi != index)[0]
    if diff.size:
        st_g = M.states_from_index(tab, index)
        for s0, s1 in M.segments(seg_start, tab["F"]):
            if s1 > s0 and np.any((diff >= s0) & (diff < s1)):
                a, b = M.path_score(tab, st_m, s0, s1), M.path_score(tab, st_g, s0, s1)
                assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1.0), (name, s0, s1, a, b)
    REPORT.setdefault("near_tie_frames", {})[name] = int(diff.size)
    return int(diff.size)


# ---- hand-built lists with known answers -------------------------------------------------------------------------------------

def test_octave_alternation_stays_on_f0(vb, pkg):
    """The top candidate alternates between f0 and 2 f0; the per-frame argmax jumps an octave every frame, the path stays on f0."""
    F = 50
    cand = np.zeros((F, 2, 2))
    for t in range(F):
        cand[t] = [[200.0, 0.85], [400.0, 0.78]] if t % 2 == 0 else [[400.0, 0.82], [200.0, 0.80]]
    count = np.full(F, 2, np.int32)
    path, index = _run(vb, pkg, cand, count, silence_threshold=0.0)
    assert np.all(path[:, 0] == 200.0)
    assert np.array_equal(index, np.where(np.arange(F) % 2 == 0, 0, 1))
    _check_against_model(cand, count, None, None, None, (path, index), "octave", silence_threshold=0.0)


def test_one_frame_dropout_is_bridged(vb, pkg):
    F = 40
    cand = np.tile(np.array([[[200.0, 0.9]]]), (F, 1, 1))
    cand[10, 0] = [200.0, 0.35]                                # alone, the unvoiced state (0.45) beats it
    count = np.ones(F, np.int32)
    path, index = _run(vb, pkg, cand, count, silence_threshold=0.0)
    assert np.all(index == 0) and np.all(path[:, 0] == 200.0)
    assert path[10, 1] == 0.35
    _check_against_model(cand, count, None, None, None, (path, index), "dropout", silence_threshold=0.0)


def test_quiet_frames_go_unvoiced(vb, pkg):
    F = 60
    cand = np.tile(np.array([[[200.0, 0.6]]]), (F, 1, 1))
    count = np.ones(F, np.int32)
    lp = np.ones(F)
    lp[20:30] = 0.001
    path, index = _run(vb, pkg, cand, count, local_peak=lp)
    assert np.all(index[20:30] == -1) and np.all(path[20:30, 0] == 0.0)
    assert np.all(index[:20] == 0) and np.all(index[30:] == 0)
    q = 0.03 / (1.0 + 0.45)
    assert np.array_equal(path[20:30, 1], 0.45 + (2.0 - (lp[20:30] / 1.0) / q))      # u_t, bit for bit
    _check_against_model(cand, count, None, lp, None, (path, index), "quiet")


def test_ties_go_to_the_lower_index(vb, pkg):
    F = 30
    cand = np.tile(np.array([[[200.0, 0.7], [200.0, 0.7], [300.0, 0.1]]]), (F, 1, 1))
    count = np.full(F, 3, np.int32)
    path, index = _run(vb, pkg, cand, count, silence_threshold=0.0)
    assert np.all(index == 0)
    _check_against_model(cand, count, None, None, None, (path, index), "ties", silence_threshold=0.0)


def test_kmax_1_with_the_appended_unvoiced_state(vb, pkg):
    F = 30
    cand = np.tile(np.array([[[220.0, 0.9]]]), (F, 1, 1))
    count = np.ones(F, np.int32)
    count[5:15] = 0                                            # no listed state: only the appended one
    cand[20:25, 0] = [0.0, 0.5]                                # a listed unvoiced state: nothing is appended
    path, index = _run(vb, pkg, cand, count, silence_threshold=0.0)
    assert np.all(index[5:15] == -1) and np.all(path[5:15] == [0.0, 0.45])
    assert np.all(index[20:25] == 0) and np.all(path[20:25] == [0.0, 0.45])
    assert np.all(index[:5] == 0) and np.all(path[:5, 0] == 220.0)
    _check_against_model(cand, count, None, None, None, (path, index), "kmax1", silence_threshold=0.0)


def test_frames_not_ok_are_unvoiced(vb, pkg):
    F = 30
    cand = np.tile(np.array([[[220.0, 0.9], [110.0, 0.5]]]), (F, 1, 1))
    count = np.full(F, 2, np.int32)
    status = np.zeros(F, np.int32)
    status[[3, 4, 17]] = [3, 1, 4]
    path, index = _run(vb, pkg, cand, count, status, silence_threshold=0.0)
    assert np.all(index[[3, 4, 17]] == -1) and np.all(path[[3, 4, 17], 0] == 0.0)
    assert np.sum(index == -1) == 3
    _check_against_model(cand, count, status, None, None, (path, index), "status", silence_threshold=0.0)


def test_one_frame_segments_and_a_single_frame(vb, pkg):
    rng = np.random.default_rng(7)
    F, kmax = 500, 4
    cand = np.stack([rng.uniform(75, 600, (F, kmax)), rng.uniform(0, 1, (F, kmax))], axis=-1)
    count = rng.integers(0, kmax + 2, F).astype(np.int32)
    lp = rng.uniform(0, 1, F)
    seg = np.arange(F, dtype=np.int64)
    got = _run(vb, pkg, cand, count, local_peak=lp, seg_start=seg)
    assert _check_against_model(cand, count, None, lp, seg, got, "one_frame_segments") == 0
    # one frame per segment: the path is each frame's best lambda (with every P the frame's own peak: rho = 1)
    tab = M.frame_table(cand, count, None, lp, seg, M.DEFAULTS)
    best = np.argmax(np.where(tab["active"], tab["lam"], -np.inf), axis=1)
    assert np.array_equal(M.states_from_index(tab, got[1]), best)
    one = _run(vb, pkg, cand[:1], count[:1], local_peak=lp[:1])
    assert np.array_equal(one[1], got[1][:1]) and np.array_equal(one[0], got[0][:1])


# ---- against the model ---------------------------------------------------------------------------------------------------------

def _random_lists(rng, F, kmax, zero_frac=0.1):
    f = rng.uniform(60.0, 650.0, (F, kmax))
    f[rng.uniform(size=(F, kmax)) < zero_frac] = 0.0
    a = rng.uniform(0.0, 1.0, (F, kmax))
    cand = np.stack([f, a], axis=-1)
    count = rng.integers(0, kmax + 3, F).astype(np.int32)
    status = np.where(rng.uniform(size=F) < 0.03, rng.integers(1, 5, F), 0).astype(np.int32)
    lp = rng.uniform(0.0, 1.0, F) ** 3
    return cand, count, status, lp


@pytest.mark.parametrize("kmax,n_seg", [(2, 10000), (4, 10000), (8, 10000), (15, 10000), (63, 500)])
def test_random_lists_match_the_model(vb, pkg, kmax, n_seg):
    rng = np.random.default_rng(1000 + kmax)
    L = 400
    F = n_seg * L
    cand, count, status, lp = _random_lists(rng, F, kmax)
    seg = np.arange(0, F, L, dtype=np.int64)
    got = _run(vb, pkg, cand, count, status, lp, seg)
    n = _check_against_model(cand, count, status, lp, seg, got, f"random_k{kmax}")
    assert n <= F // 100000 + 1                                # expected 0: a differing frame needs a score tie within 1e-12


def _read_wav16(path):
    with wave.open(path, "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        return pcm.astype(np.float64) / 32767.0, float(w.getframerate())


@pytest.mark.parametrize("name", ["short_sample", "down_sampled", "sample-two_vowels"])
def test_golden_speech_lists_match_the_model(vb, pkg, golden_dir, name):
    x, sr = _read_wav16(os.path.join(golden_dir, name + ".wav"))
    n, hop = 1024, 256
    F = pkg.frame_count(x.size, n, hop)
    win = vb.window(pkg.WINDOW_HANNING, n)
    for kmax in (4, 15):
        cand, count, status = vb.pitch(x, sr, 0.2, 75.0, 600.0, kmax=kmax, frame_len=n, stride=hop, window=win)
        lp = vb.frame_peak(x, frame_len=n, stride=hop)
        kw = dict(time_step=hop / sr)
        got = _run(vb, pkg, cand, count, status, lp, None, **kw)
        assert _check_against_model(cand, count, status, lp, None, got, f"{name}_k{kmax}", **kw) == 0
        assert np.any(got[1] >= 0)                             # voiced somewhere
    # the one-call chain gives the same path
    tr = vb.pitch_track(x, sr, 75.0, 600.0, kmax=15, frame_len=n, stride=hop)
    assert np.array_equal(tr[1], got[1]) and np.array_equal(tr[0].view(np.int64), got[0].view(np.int64))


def test_synth_speech_lists_match_the_model(vb, pkg):
    N, H, SR = 1200, 480, 48000.0
    F = 20000
    audio = vb.synth_speech((F - 1) * H + N, sample_offset=7 * 48000)
    win = vb.window(pkg.WINDOW_HANNING, N)
    for kmax in (4, 15):
        cand, count, status = vb.pitch(audio, SR, 0.2, 75.0, 600.0, kmax=kmax, frame_len=N, stride=H, n_frames=F, window=win)
        lp = vb.frame_peak(audio, frame_len=N, stride=H, n_frames=F)
        seg = np.arange(0, F, 5000, dtype=np.int64)
        got = _run(vb, pkg, cand, count, status, lp, seg)
        assert _check_against_model(cand, count, status, lp, seg, got, f"synth_k{kmax}") == 0
        assert np.mean(got[1] >= 0) > 0.3                      # voiced speech
    audio.free()


# ---- chunked == sequential, bit for bit -----------------------------------------------------------------------------------------

def _both(vb, pkg, cand_d, cnt_d, st_d, lp_d, F, kmax, seg=None, **kw):
    outs = []
    for chunk in (0, F):
        p = _params(pkg, chunk_frames=chunk, **kw)
        path, idx = vb.empty((F, 2)), vb.empty(F, np.int32)
        vb.pitch_path(cand_d, cnt_d, st_d, lp_d, seg_start=seg, params=p, n_frames=F, kmax=kmax, out=(path, idx))
        redone = vb.last_path_chunks_redone()
        outs.append((path.numpy(), idx.numpy(), redone))
        path.free(); idx.free()
    return outs


def test_chunked_equals_sequential_on_the_bench_utterance(vb, pkg):
    """The bench's 4.5 M-frame single utterance (1200 / 480 at 48 kHz, 12.5 h), kmax 4, lists built in pieces."""
    N, H, SR, F, kmax = 1200, 480, 48000.0, 4_500_000, 4
    piece = 450_000
    cand_d, cnt_d, st_d, lp_d = vb.empty((F, kmax, 2)), vb.empty(F, np.int32), vb.empty(F, np.int32), vb.empty(F)
    win = vb.window(pkg.WINDOW_HANNING, N)
    audio = vb.empty((piece - 1) * H + N)
    for p0 in range(0, F, piece):
        vb.synth_speech((piece - 1) * H + N, sample_offset=p0 * H, out=audio)
        vb.pitch(audio, SR, 0.2, 75.0, 600.0, kmax=kmax, frame_len=N, stride=H, n_frames=piece, window=win,
                 out=(cand_d.ptr + p0 * kmax * 16, cnt_d.ptr + p0 * 4, st_d.ptr + p0 * 4))
        vb.frame_peak(audio, frame_len=N, stride=H, n_frames=piece, out=lp_d.ptr + p0 * 8)
    audio.free()
    (pc, ic, rc), (ps, is_, rs) = _both(vb, pkg, cand_d, cnt_d, st_d, lp_d, F, kmax)
    assert np.array_equal(ic, is_)
    assert np.array_equal(pc.view(np.int64), ps.view(np.int64))
    assert rs == 0
    REPORT["bench_utterance"] = dict(frames=F, chunks_redone=rc, voiced=float(np.mean(ic >= 0)))
    for d in (cand_d, cnt_d, st_d, lp_d):
        d.free()


def _adversarial(F, seed=3):
    """Two near-equal tracks half an octave apart: their score difference is a random walk far inside the switching cost, so the
    non-leader's D keeps the whole history (nothing is forgotten) and every warm-up guess is wrong."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1e-4, 1e-4, F)
    cand = np.zeros((F, 2, 2))
    cand[:, 0] = np.stack([np.full(F, 200.0), 0.7 + d / 2], axis=-1)
    cand[:, 1] = np.stack([np.full(F, 200.0 * 2 ** 0.5), 0.7 - d / 2 - 0.005], axis=-1)   # -0.005: its octave cost is lower
    return cand, np.full(F, 2, np.int32)


def test_chunked_equals_sequential_on_an_adversarial_stream(vb, pkg):
    F, kmax = 40000, 2
    cand, count = _adversarial(F)
    cand_d, cnt_d = vb.to_device(cand), vb.to_device(count)
    (pc, ic, rc), (ps, is_, rs) = _both(vb, pkg, cand_d, cnt_d, None, None, F, kmax, seg=np.array([0, 15000], np.int64),
                                          silence_threshold=0.0)
    assert rc > 0, "the repair rounds / sweep never ran"
    assert rs == 0
    assert np.array_equal(ic, is_)
    assert np.array_equal(pc.view(np.int64), ps.view(np.int64))
    REPORT["adversarial"] = dict(frames=F, chunks_redone=rc)
    cand_d.free(); cnt_d.free()


# ---- frame peak, errors, profiler ---------------------------------------------------------------------------------------------

def test_frame_peak_is_nanmax(vb, pkg):
    rng = np.random.default_rng(5)
    x = rng.normal(size=200000)
    x[rng.uniform(size=x.size) < 0.01] = np.nan
    x[1200:2400] = np.nan                                      # frame 5 (stride 240) holds nothing else
    for n, hop in ((1200, 240), (4096, 1000), (5000, 4999), (1, 1)):
        F = pkg.frame_count(x.size, n, hop)
        got = vb.frame_peak(x, frame_len=n, stride=hop)
        fr = np.lib.stride_tricks.sliding_window_view(x, n)[::hop][:F]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # the all-NaN frame
            exp = np.nanmax(np.abs(fr), axis=1)
        assert np.array_equal(np.isnan(got), np.isnan(exp))
        ok = ~np.isnan(exp)
        assert np.array_equal(got[ok].view(np.int64), exp[ok].view(np.int64))


def test_invalid_arguments_leave_the_context_usable(vb, pkg):
    rng = np.random.default_rng(11)
    F, kmax = 3000, 4
    cand, count, status, lp = _random_lists(rng, F, kmax)
    d = [vb.to_device(cand), vb.to_device(count), vb.to_device(status), vb.to_device(lp)]
    path, idx = vb.empty((F, 2)), vb.empty(F, np.int32)
    L = vb.L

    def call(k=kmax, params=None, lp_ptr=d[3].ptr, seg=None, n_seg=0):
        p = params if params is not None else _params(pkg)
        return L.vbx_pitch_path_f64(vb.ctx, d[0].ptr, d[1].ptr, d[2].ptr, F, k, lp_ptr, seg, n_seg, C.byref(p), path.ptr, idx.ptr)

    bad = [dict(k=0), dict(k=64)]
    for field in ("voicing_threshold", "silence_threshold", "octave_cost", "octave_jump_cost", "voiced_unvoiced_cost",
                  "ceiling_hz", "time_step"):
        for v in (-0.1, float("nan"), float("inf")):
            p = _params(pkg); setattr(p, field, v); bad.append(dict(params=p))
    for field in ("time_step", "ceiling_hz"):
        p = _params(pkg); setattr(p, field, 0.0); bad.append(dict(params=p))
    bad.append(dict(lp_ptr=None))                              # silence_threshold 0.03 > 0 without local_peak
    for s in ([1, 5], [0, 9, 5], [0, F + 1]):
        a = np.array(s, np.int64)
        bad.append(dict(seg=a.ctypes.data, n_seg=a.size, _keep=a))
    for b in bad:
        kw = {k: v for k, v in b.items() if k != "_keep"}
        assert call(**kw) == -1, b                             # VBX_E_INVALID
        assert vb.last_path_chunks_redone() == -1
    # the next valid call is right, and the inputs are untouched
    assert call() == 0
    got = (path.numpy(), idx.numpy())
    assert _check_against_model(cand, count, status, lp, None, got, "after_errors") == 0
    for dev, host in zip(d, (cand, count, status, lp)):
        assert np.array_equal(dev.numpy().view(np.uint8), np.ascontiguousarray(host).view(np.uint8))
    for x in d + [path, idx]:
        x.free()


def test_every_kernel_is_profiled(vb, pkg):
    F, kmax = 40000, 2
    cand, count = _adversarial(F, seed=9)
    lp = np.linspace(0.1, 1.0, F)
    vb.profile(True)
    vb.profile_reset()
    try:
        vb.frame_peak(np.zeros(4800), frame_len=1200, stride=480)
        vb.pitch_path(cand, count, None, lp, params=_params(pkg))
        rep = vb.profile_report()
    finally:
        vb.profile(False)
    for name in ("frame_peak", "pitch_path_peak", "pitch_path_spec", "pitch_path_check", "pitch_path_repair", "pitch_path_sweep",
                 "pitch_path_backtrack", "pitch_path_compose", "pitch_path_write"):
        assert name in rep and rep[name][1] >= 1, (name, sorted(rep))


def test_report():
    print("pitch path report:", REPORT)
