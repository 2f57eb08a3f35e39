"""Calls larger than one launch's scratch: every host loop that cuts a call's frames into several launches is crossed at its production
size, and every capped grid takes a second trip, on a real MI355X (`-m gpu`).

How a call of 265,000 frames is held row by row: the audio repeats with a period of K = 211 frames (tests/periodic_frames.py), so row
f + K must equal row f bit for bit -- one download, one vectorised comparison -- and the first rows are held to a reference: the same
entry point on the first frames alone (one launch; the split form: the fused kernel of a context created under VBX_POW2_SPLIT=0), bit
for bit, and the CPU oracle on a handful at the project's tolerances (rel_close 1e-6, Hz 1e-4 through classify_top, counts and statuses
exact).  Outputs carry K canary rows past F.  That a seam was crossed, and the batch size, come from vbx_internal_last_batching -- never
from a restated formula; F is sized from PER_GUESS below and the assertion is on the probe.  The batch size is never a multiple of K
(asserted), so a batch's stale scratch cannot line up with the period.

Inventory: the host loops of csrc/ that cut a call's frames (or items) into several launches, and the kernels whose grid is capped
(they stride over the rest).  cap = frames (elements) per launch (trip); then the smallest call that crosses it and the test that does.

  host loops
    launch_pow2_u, vbx_spectral_pow2.hpp (the 4096-point plan as two kernels; scratch sized in launch_spectral, vbx_api.hip)
        cap just above 131,072 frames (probe)      analyze_frames / pitch, 2049..4096 samples, more frames than that      test_split_form_*
    run_pitch, vbx_api.hip (frames beyond 4096 samples)
        2^31 / scratch bytes per frame: 17,451 at 4097 samples                                                            test_long_pitch
    run_burg, vbx_api.hip (frames beyond 4096 samples)
        2^30 / scratch bytes per frame: 8,190 at 4097 samples                                                             test_long_burg_and_find_formants
    run_burg, vbx_api.hip (the dense resampled fallback)
        256 MiB / resampled frame: 16,384 at m = 2048                                                                     test_dense_resampled_fallback
    vbx_lpc_burg_f32, vbx_api_f32.hip
        256 MiB / (8 frame_len), a multiple of 64: 8,192 at 4096 samples                                                  test_f32_burg
    run_burg, vbx_api.hip (burg_fast_chunk: items of the one-pass lag kernel)
        524,288 frames                               tests/test_gpu_full_size.py (config 4, one million frames)
    launch_spectral, vbx_api.hip (analyze launches leaving Burg's lag sums)
        VBX_ANALYZE_LAUNCH_FRAMES (524,288)          tests/test_gpu_burg_fused.py (lowered to 1000), tests/test_gpu_full_size.py
    run_find_formants, vbx_api.hip (the tracker's time slices)
        utterance length / 6, from 65,536 frames in >= 64 utterances         tests/test_gpu_regressions.py, tests/test_gpu_tracker_chunked.py
    vbx_analyze_host* (host chunk plan), vbx_analyze_clips (clip groups), the pitch path's chunks
        the caller's chunk_frames / group_frames     tests/test_gpu_analyze_host.py, tests/test_gpu_clips.py, tests/test_gpu_pitch_path.py
  capped grids (blocks of 256 threads unless said)
    pcm16_kernel, k_front.hip                  8,192 blocks, two samples a thread: 4,194,304 samples          test_pcm16_to_f64_past_the_capped_grid
    resample_kernel, k_front.hip               8,192: 2,097,152 resampled samples (1,025 frames at m = 2048)  test_dense_resampled_fallback
    ring_frames_kernel, k_front.hip            65,536: 16,777,216 elements                                     test_ring_frames_past_the_capped_grid
    widen_frames_kernel, narrow_kernel         65,536: 16,777,216 elements                                     test_f32_wide_past_the_capped_grids
    autocorr_long_finish_kernel, k_long.hip    8,192: 2,097,152 lag entries (512 frames at 4097 lags)          test_long_pitch
    pitch_long_curve_kernel, k_long.hip        16,384: 4,194,304 curve entries (512 frames at 4097 samples)    test_long_pitch
    refine_far_kernel, k_spectral_pow2.hip     2,048 blocks of 64 over a device-side list                      test_split_form_* (a grid over a count, not over F)
    pitch_list_kernel (profiled as pitch_direct_fallback; launch_spectral, vbx_api.hip) and lpc_exact_list_kernel (vbx_lpc_exact.hpp)
                                               one or four blocks per CU over a device-side list of frames (almost always empty): no test is known
                                               to put more frames on either list than its grid holds; tests/test_gpu_parity.py
                                               (test_pitch_odd_signals) and tests/test_gpu_lpc_exact.py fill the lists, below the grid
    synth_kernel, k_synth.hip                  16,384: 4,194,304 samples                                       test_synth_speech_past_the_capped_grid
    f32_to_f64_kernel, k_front_f32in.hip       8,192, two samples a thread: 4,194,304 samples                  test_f32_to_f64_past_the_capped_grid
    unpack_kernel, k_reader.hip                8,192, 2 .. 8 samples a thread: 2,097,152 groups                test_unpack_samples_past_the_capped_grid
    unpack_all_tiled_kernel, k_reader.hip      2,048 blocks over tiles of 8 KB: 4,194,304 frames of 16-bit stereo     test_unpack_channels_past_the_capped_grids
    unpack_all_elem_kernel, k_reader.hip       8,192: 2,097,152 samples                                        test_unpack_channels_past_the_capped_grids
    mfcc_mfma_kernel, k_mfcc_mfma.hip          8 blocks per CU, up to 8 frames a block: 16,384 frames at 256 CUs      test_mfcc_kernels_past_their_block_caps
    mfcc_dft2_kernel, k_mfcc.hip               16 blocks per CU, up to 8 frames a block: 32,768 frames at 256 CUs     test_mfcc_kernels_past_their_block_caps
    host_rows_kernel, k_reader.hip             8,192: a host chunk of 2,097,152 record entries (58,255 frames of 36 columns)     test_host_chunk_rows_past_the_capped_grid
    session_ingest_kernel, k_session.hip       8,192, 2 .. 8 samples a thread: a push of 16,777,216 16-bit samples                test_session_push_past_the_capped_grids
    session_deliver_kernel, k_session.hip      8,192: a push that completes 58,255 frames of 36 columns                          test_session_push_past_the_capped_grids
    session_ingest_all_kernel, vbx_session_ingest_all.hpp      2,048 blocks over tiles of 8 KB: 4,194,304 frames of 16-bit stereo     test_session_channels_push_past_the_capped_grids
    session_deliver_all_kernel, k_session_channels.hip         1,024 per channel: a push that completes 7,282 frames of 36 columns    test_session_channels_push_past_the_capped_grids
    pool_ingest_kernel, k_pool.hip             8,192 blocks over tiles of 1,024 groups: a tick of 16,777,216 f64 samples          test_pool_tick_past_the_capped_grids
    pool_deliver_kernel, k_pool.hip            2,048: a tick that completes 29,128 frames of 36 columns                           test_pool_tick_past_the_capped_grids
    clips_pack_kernel, vbx_clips_pack.hpp      8,192 blocks over tiles of 1,024 groups: a group of 16,777,216 f64 samples         test_clip_group_past_the_capped_grids
    clips_deliver_kernel, k_clips.hip          2,048: a group of 29,128 frames of 36 columns                                      test_clip_group_past_the_capped_grids
  not crossed: the by-element side of session_ingest_all_kernel (8,192 blocks over the groups outside whole tiles: an unaligned push of
  2,097,152 groups) and the 8-bit readers' own instances of these kernels (k_sample8.hip); the instances above share their loops' shape
"""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import layout_arena as la
import parity_asserts as pa
import periodic_frames as pf
from analyze_reference import classify_top, oracle_records
from conftest import rel_close

pytestmark = pytest.mark.gpu

SR = 48000.0
K, HOP = 211, 128                                            # the period in frames; K * HOP = 27,008 samples >= three frames of 4097
OFFSET = 3 * 48000 + 12345
PITCH = (0.2, 75.0, 600.0)
MFCC = (13, 100.0, 8000.0)
ORDER = 12
MAX_RES = 32                                                 # VBX_MAX_RESONANCES: the resonance rows find_formants writes
# frames per launch as read from the code, to size F by; what is asserted comes from the probe
PER_GUESS = {"split": 131072, "long_pitch": 17451, "long_burg": 8190, "dense": 16384, "f32_burg": 8192}
F_SPLIT = 265003                                             # two crossings of a cap a few hundred above 131,072; 43 mod 64
REF_SPLIT = 2000                                             # frames of the fused kernel's reference
LONG_PITCH_CROSSINGS = 2                                     # 0.13 s measured for both at the most: see test_long_pitch
REPORT = {"cases": {}}


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
def pattern(vb):
    d = vb.synth_speech(K * HOP, sample_offset=OFFSET)
    h = d.numpy()
    d.free()
    return h


@pytest.fixture(scope="module")
def audio_split(vb, pattern):
    """(host, device) the tiled signal of the split cases: F_SPLIT frames of up to 4096 samples, 128 apart (271 MB)"""
    pf.check_period(K, HOP, 4096)
    host = pf.tiled(pattern, pf.samples_needed(F_SPLIT, HOP, 4096))
    d = vb.to_device(host)
    yield host, d
    d.free()


@pytest.fixture(scope="module")
def vb_fused(pkg):
    ctx = _ctx(pkg, {"VBX_POW2_SPLIT": "0"})
    yield ctx
    ctx.close()


def _est0(pkg):
    return np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])


def _canary(vb, dtype, rows, cols=None):
    return vb.to_device(pf.canary_rows(dtype, rows, cols))


def _timed(vb, fn):
    vb.sync()
    t0 = time.perf_counter()
    fn()
    vb.sync()
    return time.perf_counter() - t0


def _crossed(name, vb, F, want_batches, min_tail=1):
    """The probe's (batches, frames per batch) of the context's last call: the seam was crossed, the last batch is short, the batch is no
    multiple of the period, F no multiple of 64."""
    batches, per = vb.last_batching()
    assert batches >= want_batches, (name, "launches", batches, "frames per launch", per, "F", F, "-- PER_GUESS no longer fits the library")
    assert batches == -(-F // per), (name, batches, per, F)
    tail = F - (batches - 1) * per
    assert min_tail <= tail < per, (name, "the last launch has", tail, "frames of", per)
    assert F % 64 != 0 and F % per != 0
    pf.assert_batch_breaks_period(per, K)
    return batches, per


def _note(name, F, batches, per, grids, seconds, **more):
    REPORT["cases"][name] = dict(F=F, frames_per_batch=per, batches=batches, capped_grids_crossed=sorted(grids), seconds=round(seconds, 4), **more)
    print(f"\nbatch seams {name}: {REPORT['cases'][name]}")


def _same(label, name, got, want):
    la.assert_same_bits(label, name, np.ascontiguousarray(got), np.ascontiguousarray(want))


def _planes(label, st_flat, F, per):
    """status3 [3][F] (+ K canary words behind the third plane) -> [3, F]; every plane periodic, the tail untouched"""
    for q in range(3):
        rows = st_flat[q * F:(q + 1) * F + (K if q == 2 else 0)]
        pf.assert_periodic(label, f"status3[{q}]", rows, F, K, per)
    return st_flat[:3 * F].reshape(3, F)


def _check_pitch_rows(label, oracle, host, n, window, rows, kmax, cand, cnt, st):
    for f in rows:
        es, ec, en = oracle.pitch(host[f * HOP:f * HOP + n] * window, SR, *PITCH, cap=max(2, kmax))
        assert st[f] == es == 0 and cnt[f] == en, (label, f, st[f], es, cnt[f], en)
        top2 = np.zeros((2, 2))
        top2[:min(2, ec.shape[0])] = ec[:2]
        assert classify_top(cand[f, 0], top2, en) in ("ok", "swap"), (label, f, cand[f, 0], ec[:2])


# ---- 1. the 4096-point plan as two kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,what", [(4096, "even, the full transform"), (3000, "MFCC bins interpolated"), (2205, "odd: the whole curve in the scratch row")],
                         ids=["4096", "3000", "2205"])
def test_split_form_analyze(vb, vb_fused, pkg, oracle, audio_split, n, what):
    """vbx_analyze_frames_f64 (pitch + LPC + MFCC; formant_order 0: the formant chain is not what this seam cuts) on 265,003 frames: three
    launches of the transform kernel and of scan / refine / far, each over its own stretch of the scratch rows."""
    host, x_d = audio_split
    F, name = F_SPLIT, f"split-analyze-{n}"
    params = pkg.AnalysisParams.make(SR, pitch=PITCH, lpc_order=ORDER, formant_order=0, mfcc=MFCC)
    width = int(vb.L.vbx_record_doubles(C.byref(params)))
    assert width == 28
    rec_d, st_d = _canary(vb, np.float64, F + K, width), _canary(vb, np.int32, 3 * F + K)
    try:
        dt = _timed(vb, lambda: vb.analyze_frames(x_d, params, frame_len=n, stride=HOP, n_frames=F, out=rec_d, status=st_d))
        assert int(vb.L.vbx_internal_last_spectral_split(vb.ctx)) == 1, name
        batches, per = _crossed(name, vb, F, 3)
        rec, st_flat = rec_d.numpy(), st_d.numpy()
    finally:
        rec_d.free(); st_d.free()
    _note(name, F, batches, per, ["refine_far_kernel"], dt, shape=what)
    pf.assert_periodic(name, "records", rec, F, K, per)
    st = _planes(name, st_flat, F, per)
    # the first rows: the fused kernel on them alone, bit for bit
    ref_x = vb_fused.to_device(host[:pf.samples_needed(REF_SPLIT, HOP, n)])
    ref, ref_st = vb_fused.analyze_frames(ref_x, params, frame_len=n, stride=HOP, n_frames=REF_SPLIT)
    assert int(vb_fused.L.vbx_internal_last_spectral_split(vb_fused.ctx)) == 0 and vb_fused.last_batching() == (0, 0)
    ref_x.free()
    _same(name, "records[:2000]", rec[:REF_SPLIT], ref[:, :width])
    _same(name, "status3[:, :2000]", st[:, :REF_SPLIT], ref_st)
    assert np.count_nonzero(rec[:K, 0]) > K // 4                                   # voiced frames among the period's
    # and the oracle on four of the period's rows
    rows = [0, 70, 141, K - 1]
    orec, ost, top2, counts = oracle_records(oracle, host, n, HOP, rows, SR, PITCH, ORDER, 0, None, MFCC, None)
    for i, f in enumerate(rows):
        assert np.array_equal(st[:, f], ost[:, i]), (name, f)
        assert classify_top(rec[f, 0:2], top2[i], counts[i]) in ("ok", "swap"), (name, f, rec[f, 0:2], top2[i])
        assert np.all(rel_close(rec[f, 2:15], orec[i, 2:15])) and np.all(rel_close(rec[f, 15:28], orec[i, 15:28])), (name, f)


@pytest.mark.parametrize("kmax", [1, 8])
def test_split_form_pitch(vb, vb_fused, pkg, oracle, audio_split, kmax):
    """vbx_pitch_f64 at 4096 samples through the same loop: the candidate rows, counts and statuses of 265,003 frames."""
    host, x_d = audio_split
    n, F, name = 4096, F_SPLIT, f"split-pitch-kmax{kmax}"
    han = vb.window(pkg.WINDOW_HANNING, n)
    out = (_canary(vb, np.float64, F + K, 2 * kmax), _canary(vb, np.int32, F + K), _canary(vb, np.int32, F + K))
    try:
        dt = _timed(vb, lambda: vb.pitch(x_d, SR, *PITCH, kmax=kmax, frame_len=n, stride=HOP, n_frames=F, window=han, out=out))
        assert int(vb.L.vbx_internal_last_spectral_split(vb.ctx)) == 1, name
        batches, per = _crossed(name, vb, F, 3)
        cand, cnt, st = (a.numpy() for a in out)
    finally:
        for a in out:
            a.free()
    _note(name, F, batches, per, ["refine_far_kernel"], dt)
    for nm, a in (("candidates", cand), ("count", cnt), ("status", st)):
        pf.assert_periodic(name, nm, a, F, K, per)
    ref_x = vb_fused.to_device(host[:pf.samples_needed(REF_SPLIT, HOP, n)])
    rc, rn, rs = vb_fused.pitch(ref_x, SR, *PITCH, kmax=kmax, frame_len=n, stride=HOP, n_frames=REF_SPLIT, window=vb_fused.window(pkg.WINDOW_HANNING, n))
    assert int(vb_fused.L.vbx_internal_last_spectral_split(vb_fused.ctx)) == 0
    ref_x.free()
    _same(name, "candidates[:2000]", cand[:REF_SPLIT], rc.reshape(REF_SPLIT, 2 * kmax))
    _same(name, "count[:2000]", cnt[:REF_SPLIT], rn)
    _same(name, "status[:2000]", st[:REF_SPLIT], rs)
    _check_pitch_rows(name, oracle, host, n, oracle.window("hanning", n), [0, 70, 141, K - 1], kmax, cand.reshape(-1, kmax, 2), cnt, st)


# ---- 2. frames beyond 4096 samples --------------------------------------------------------------------------------------------------------

def test_long_pitch(vb, pkg, oracle, pattern):
    """vbx_pitch_f64 at 4097 samples, kmax 2: batches of the long-frame scratch.  The last batch and the reference call have at least 320
    frames: with fewer, autocorr_long_splits (k_long.hip) cuts the lag sums into more than one partial sum and the rows may differ from
    the other batches' in the last bits (that form: tests/accuracy_cases.py, the autocorr-*-long-* cases).  Each batch takes
    autocorr_long_finish_kernel and pitch_long_curve_kernel past their capped grids.

    Two crossings (F = 2 * 17,451 + 531 = 35,433 frames): the refinement runs at depth 1200 on every candidate, and the call was measured
    at 0.05 .. 0.13 s on the MI355X (profiles/batch_seams/report.json, this case's `seconds`), so a single crossing was not needed."""
    n, kmax, name = 4097, 2, "long-pitch-4097"
    pf.check_period(K, HOP, n)
    per_g = PER_GUESS["long_pitch"]
    F = LONG_PITCH_CROSSINGS * per_g + 320 + K
    host = pf.tiled(pattern, pf.samples_needed(F, HOP, n))
    x_d = vb.to_device(host)
    han = vb.window(pkg.WINDOW_HANNING, n)
    out = (_canary(vb, np.float64, F + K, 2 * kmax), _canary(vb, np.int32, F + K), _canary(vb, np.int32, F + K))
    try:
        dt = _timed(vb, lambda: vb.pitch(x_d, SR, *PITCH, kmax=kmax, frame_len=n, stride=HOP, n_frames=F, window=han, out=out))
        batches, per = _crossed(name, vb, F, LONG_PITCH_CROSSINGS + 1, min_tail=320)
        cand, cnt, st = (a.numpy() for a in out)
        assert int(vb.L.vbx_internal_last_pitch_form(vb.ctx)) == 100
        # the capped grids of every batch, the short last one included: the arithmetic, not a comment
        tail = F - (batches - 1) * per
        assert tail * n > 8192 * 256 and tail * 2 * n > 16384 * 256
        ref_F = 320 + K
        rc, rn, rs = vb.pitch(x_d, SR, *PITCH, kmax=kmax, frame_len=n, stride=HOP, n_frames=ref_F, window=han)
        assert vb.last_batching() == (1, ref_F)
    finally:
        for a in out + (x_d,):
            a.free()
    _note(name, F, batches, per, ["autocorr_long_finish_kernel", "pitch_long_curve_kernel"], dt, crossings=LONG_PITCH_CROSSINGS)
    for nm, a in (("candidates", cand), ("count", cnt), ("status", st)):
        pf.assert_periodic(name, nm, a, F, K, per)
    _same(name, "candidates[:531]", cand[:ref_F], rc.reshape(ref_F, 2 * kmax))
    _same(name, "count[:531]", cnt[:ref_F], rn)
    _same(name, "status[:531]", st[:ref_F], rs)
    _check_pitch_rows(name, oracle, host, n, oracle.window("hanning", n), [0, 30, 60, 90, 120, 150, 180, K - 1], kmax, cand.reshape(-1, kmax, 2), cnt, st)


def test_long_burg_and_find_formants(vb, pkg, oracle, pattern):
    """vbx_lpc_burg_f64 and vbx_find_formants_f64 at 4097 samples, order 12: batches of the long-frame Burg's L2-resident scratch.  Every
    period is an utterance, so the tracked formants repeat too; F stays below the 65,536 frames from which the tracker runs in time
    slices (tests/test_gpu_regressions.py)."""
    n, name = 4097, "long-burg-4097"
    F = 2 * PER_GUESS["long_burg"] + 300
    assert F < 65536
    host = pf.tiled(pattern, pf.samples_needed(F, HOP, n))
    x_d = vb.to_device(host)
    est0 = _est0(pkg)
    seg = np.arange(0, F, K, dtype=np.int64)
    ref_F = 2 * K
    co_d, st_d = _canary(vb, np.float64, F + K, ORDER), _canary(vb, np.int32, F + K)
    bufs = {"formants": _canary(vb, np.float64, F + K, 2 * est0.shape[0]), "res": _canary(vb, np.float64, F + K, 2 * MAX_RES),
            "count": _canary(vb, np.int32, F + K), "coeffs": _canary(vb, np.float64, F + K, ORDER), "status": _canary(vb, np.int32, F + K)}
    try:
        dt = _timed(vb, lambda: vb.lpc_praat(x_d, ORDER, frame_len=n, stride=HOP, n_frames=F, out=(co_d, st_d)))
        batches, per = _crossed(name, vb, F, 3)
        co, st = co_d.numpy(), st_d.numpy()
        dt_ff = _timed(vb, lambda: vb.find_formants(x_d, SR, ORDER, est0, seg_start=seg, frame_len=n, stride=HOP, n_frames=F, out=bufs))
        assert _crossed(name + "/find_formants", vb, F, 3) == (batches, per)
        ff = {k: v.numpy() for k, v in bufs.items()}
        rco, rst = vb.lpc_praat(x_d, ORDER, frame_len=n, stride=HOP, n_frames=ref_F)
        assert vb.last_batching() == (1, ref_F)
        rff = vb.find_formants(x_d, SR, ORDER, est0, seg_start=seg[:2], frame_len=n, stride=HOP, n_frames=ref_F)
    finally:
        for a in [co_d, st_d, x_d] + list(bufs.values()):
            a.free()
    _note(name, F, batches, per, [], dt)
    _note(name + "/find_formants", F, batches, per, [], dt_ff, utterances=int(seg.size))
    pf.assert_periodic(name, "coefficients", co, F, K, per)
    pf.assert_periodic(name, "status", st, F, K, per)
    _same(name, "coefficients[:422]", co[:ref_F], rco)
    _same(name, "status[:422]", st[:ref_F], rst)
    rows = [0, 30, 60, 90, 120, 150, 180, K - 1]
    pa.burg_rows(oracle, np.stack([host[f * HOP:f * HOP + n] for f in rows]), ORDER, co[rows], st[rows], what=name)
    # find_formants: raw coefficients, resonances, counts, statuses and the tracked rows
    cnt = ff["count"]
    pf.assert_periodic(name, "find_formants count", cnt, F, K, per)
    res = ff["res"].reshape(F + K, MAX_RES, 2)
    live = np.arange(MAX_RES)[None, :] < np.clip(cnt[:F], 0, MAX_RES)[:, None]
    for nm in ("formants", "coeffs", "status"):
        pf.assert_periodic(name, "find_formants " + nm, ff[nm], F, K, per)
    _periodic_resonances(name, res, live, F, per)
    for nm in ("formants", "coeffs", "count", "status"):
        _same(name, f"find_formants {nm}[:422]", ff[nm][:ref_F].reshape(rff[nm].shape), rff[nm])
    _same_resonances(name, res[:ref_F], live[:ref_F], rff["res"])
    est = est0.copy()
    for f in range(8):                                                              # the utterance's first frames, the estimates carried
        s, est, eres, eco = oracle.find_formants(host[f * HOP:f * HOP + n], SR, ORDER, est)
        assert ff["status"][f] == s == 0, (name, f)
        _oracle_resonances(name, f, res[f], cnt[f], eres)
        assert np.all(rel_close(ff["coeffs"][f], eco)), (name, f)
        got = ff["formants"][f].reshape(-1, 2)
        assert np.all(np.abs(got[:, 0] - est[:, 0]) <= 1e-4 * np.abs(est[:, 0])), (name, f, got, est)


def _periodic_resonances(name, res, live, F, per):
    """The resonance rows [F + K, MAX_RESONANCES, 2]: the entries below the row's count are written and periodic; the rows past F keep their
    canary.  (Entries at and beyond the count are not part of the result: vbx_find_formants_f64 documents `count` entries per row.)"""
    masked = res.copy()
    masked[:F][~live] = 0.0
    pf.assert_periodic(name, "find_formants resonances", masked.reshape(res.shape[0], -1), F, K, per)


def _same_resonances(name, res, live, ref):
    """The entries below each row's count against the reference call's (whose counts were compared already), bit for bit."""
    ref = np.asarray(ref).reshape(res.shape)
    la.assert_same_bits(name, "find_formants resonances[:422]", np.ascontiguousarray(res[live]), np.ascontiguousarray(ref[live]))


def _oracle_resonances(name, f, row, count, eres):
    """One row against the oracle's resonances, as tests/test_gpu_parity.py holds them: the count exact, every entry within 1e-4."""
    n_res = int(np.sum(eres[:, 0] != 0.0))
    assert count == n_res, (name, f, count, n_res)
    assert np.all(np.abs(row[:n_res] - eres[:n_res]) <= 1e-4 * np.abs(eres[:n_res]) + 1e-9), (name, f, row[:n_res], eres[:n_res])


# ---- 3. Burg on the resampled frame: the dense fallback ----------------------------------------------------------------------------------

SILENT_AT, TONE_AT = 60, 130                                 # frames of the pattern replaced by silence and by a pure tone


@pytest.fixture(scope="module")
def pattern_special(pattern):
    p = pattern.copy()
    n = 4096
    assert TONE_AT * HOP + n <= p.size and SILENT_AT * HOP + n <= TONE_AT * HOP
    p[SILENT_AT * HOP:SILENT_AT * HOP + n] = 0.0
    p[TONE_AT * HOP:TONE_AT * HOP + n] = 0.5 * np.sin(2.0 * np.pi * 220.0 * np.arange(n) / SR)
    return p


def test_dense_resampled_fallback(vb, pkg, oracle, pattern_special):
    """vbx_find_formants_resampled_f64 and vbx_analyze_frames_ex_f64 at 4096 samples, ratio 0.5 (m = 2048), order 12: the frames are
    resampled into a context-owned dense batch of 16,384 frames at a time and take the plain one-pass Burg.  The pattern holds a silent frame
    and a pure tone, so rows leave the one-pass guard in every batch, and last_burg_direct_count must be the first K rows' count times
    F / K, exactly: launch_count_accumulate's "first batch" flag.  The resample kernel's capped grid (8,192 blocks) is crossed by every
    batch: 16,384 * 2,048 resampled samples against 2,097,152 a trip."""
    n, ratio, name = 4096, 0.5, "dense-resampled-4096"
    q = 2 * PER_GUESS["dense"] // K + 1
    F = q * K                                                                       # whole periods: the guard's count scales exactly
    host = pf.tiled(pattern_special, pf.samples_needed(F, HOP, n))
    x_d = vb.to_device(host)
    est0 = _est0(pkg)
    seg = np.arange(0, F, K, dtype=np.int64)
    rate = SR * ratio
    assert int(vb.L.vbx_resampled_len(n, ratio)) == 2048
    bufs = {"formants": _canary(vb, np.float64, F + K, 2 * est0.shape[0]), "res": _canary(vb, np.float64, F + K, 2 * MAX_RES),
            "count": _canary(vb, np.int32, F + K), "coeffs": _canary(vb, np.float64, F + K, ORDER), "status": _canary(vb, np.int32, F + K)}
    params = pkg.AnalysisParams.make(SR, pitch=PITCH, lpc_order=ORDER, formant_order=ORDER, est_init=est0, mfcc=MFCC)
    ext = pkg.AnalysisExt.make(ratio, rms=True)
    width = int(vb.L.vbx_record_doubles_ex(C.byref(params), C.byref(ext)))
    assert width == 37
    rec_d, st3_d = _canary(vb, np.float64, F + K, width + 1), _canary(vb, np.int32, 3 * F + K)
    try:
        dt = _timed(vb, lambda: vb.find_formants(x_d, rate, ORDER, est0, seg_start=seg, frame_len=n, stride=HOP, n_frames=F, out=bufs, resample_ratio=ratio))
        batches, per = _crossed(name, vb, F, 3)
        assert per * 2048 > 8192 * 256 and (F - (batches - 1) * per) * 2048 <= 8192 * 256      # (the short batch alone would not cross it)
        direct = vb.last_burg_direct_count()
        ff = {k: v.numpy() for k, v in bufs.items()}
        dt_ex = _timed(vb, lambda: vb.analyze_frames_ex(x_d, params, ext, seg_start=seg, frame_len=n, stride=HOP, n_frames=F, out=rec_d, status=st3_d, record_ld=width + 1))
        assert _crossed(name + "/analyze_ex", vb, F, 3) == (batches, per)
        direct_ex = vb.last_burg_direct_count()
        rec, st3_flat = rec_d.numpy(), st3_d.numpy()
        # the first K rows alone, and the first two periods alone (one batch each)
        r1 = vb.find_formants(x_d, rate, ORDER, est0, seg_start=seg[:1], frame_len=n, stride=HOP, n_frames=K, resample_ratio=ratio)
        direct_K = vb.last_burg_direct_count()
        assert vb.last_batching() == (1, K)
        ref_F = 2 * K
        rff = vb.find_formants(x_d, rate, ORDER, est0, seg_start=seg[:2], frame_len=n, stride=HOP, n_frames=ref_F, resample_ratio=ratio)
        rrec, rst3 = vb.analyze_frames_ex(x_d, params, ext, seg_start=seg[:2], frame_len=n, stride=HOP, n_frames=ref_F, record_ld=width + 1)
    finally:
        for a in [x_d, rec_d, st3_d] + list(bufs.values()):
            a.free()
    _note(name, F, batches, per, ["resample_kernel"], dt, burg_direct_count=direct, of_the_first_period=direct_K)
    _note(name + "/analyze_ex", F, batches, per, ["resample_kernel"], dt_ex, burg_direct_count=direct_ex)
    assert direct_K >= 2 and r1["status"][SILENT_AT] == pkg.FRAME_ERR_LPC, (direct_K, r1["status"][SILENT_AT])
    assert direct == q * direct_K and direct_ex == q * direct_K, (direct, direct_ex, q, direct_K)
    cnt = ff["count"]
    for nm in ("formants", "coeffs", "count", "status"):
        pf.assert_periodic(name, "find_formants " + nm, ff[nm], F, K, per)
        _same(name, f"find_formants {nm}[:422]", ff[nm][:ref_F].reshape(rff[nm].shape), rff[nm])
    res = ff["res"].reshape(F + K, MAX_RES, 2)
    live = np.arange(MAX_RES)[None, :] < np.clip(cnt[:F], 0, MAX_RES)[:, None]
    _periodic_resonances(name, res, live, F, per)
    _same_resonances(name, res[:ref_F], live[:ref_F], rff["res"])
    pf.assert_periodic(name, "records", rec, F, K, per, written_words=width)
    st3 = _planes(name, st3_flat, F, per)
    _same(name, "records[:422]", rec[:ref_F, :width], rrec[:, :width])
    _same(name, "status3[:, :422]", st3[:, :ref_F], rst3)
    _same(name, "the call's formant columns and find_formants' rows", rec[:F, 2:10], ff["formants"][:F])
    est = est0.copy()
    for f in range(8):
        s, est, eres, eco = oracle.find_formants(oracle.resample_linear(host[f * HOP:f * HOP + n], ratio), rate, ORDER, est)
        assert ff["status"][f] == s == 0, (name, f)
        _oracle_resonances(name, f, res[f], cnt[f], eres)
        assert np.all(rel_close(ff["coeffs"][f], eco)), (name, f)
        got = ff["formants"][f].reshape(-1, 2)
        assert np.all(np.abs(got[:, 0] - est[:, 0]) <= 1e-4 * np.abs(est[:, 0])), (name, f, got, est)


# ---- 4. vbx_lpc_burg_f32 -------------------------------------------------------------------------------------------------------------------

def test_f32_burg(vb, oracle, pattern):
    """The reference-faithful f32 Burg, a lane per frame with b1 / b2 in a scratch of 8,192 frames at 4096 samples: three launches.  The
    first period against the f32 restatement, bit for bit.  (The wide form has no loop.)"""
    n, name = 4096, "f32-burg-4096"
    F = 2 * PER_GUESS["f32_burg"] + 37
    host = pf.tiled(pattern.astype(np.float32), pf.samples_needed(F, HOP, n))
    x_d = vb.to_device(host, np.float32)
    co_d, st_d = _canary(vb, np.float32, F + K, ORDER), _canary(vb, np.int32, F + K)
    try:
        dt = _timed(vb, lambda: vb._check(vb.L.vbx_lpc_burg_f32(vb.ctx, x_d.ptr, F, n, HOP, None, ORDER, co_d.ptr, st_d.ptr)))
        batches, per = _crossed(name, vb, F, 3)
        co, st = co_d.numpy(), st_d.numpy()
    finally:
        for a in (x_d, co_d, st_d):
            a.free()
    _note(name, F, batches, per, [], dt)
    pf.assert_periodic(name, "coefficients", co, F, K, per)
    pf.assert_periodic(name, "status", st, F, K, per)
    x32 = np.stack([host[f * HOP:f * HOP + n] for f in range(K)])
    pa.burg_f32_rows(oracle, x32, ORDER, co[:K], st[:K], what=name)


# ---- 5. the capped grids ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4194304 + 3, 8388608 + 5])
def test_pcm16_to_f64_past_the_capped_grid(vb, n):
    """pcm16_kernel: 8,192 blocks of 256 threads, two samples a thread -- a second trip from 4,194,304 samples, a third from 8,388,608; the
    odd tail sample after the pairs.  Every element against int16 / 32767."""
    pcm = np.random.default_rng(n).integers(-32768, 32768, n).astype(np.int16)
    pcm[:4] = (-32768, 32767, 0, -1)
    out_d = _canary(vb, np.float64, n + K)
    try:
        src = vb.to_device(pcm, np.int16)
        dt = _timed(vb, lambda: vb._check(vb.L.vbx_pcm16_to_f64(vb.ctx, src.ptr, n, out_d.ptr)))
        got = out_d.numpy()
        src.free()
    finally:
        out_d.free()
    _note(f"pcm16-{n}", n, None, None, ["pcm16_kernel"], dt, trips=-(-(n // 2) // (8192 * 256)))
    assert n // 2 > 8192 * 256
    assert not la.unwritten(got[:n]).size and la.unwritten(got[n:]).shape[0] == K
    _same(f"pcm16-{n}", "samples", got[:n], pcm.astype(np.float64) / 32767.0)


def test_ring_frames_past_the_capped_grid(vb):
    """ring_frames_kernel: 65,536 blocks -- a second trip from 16,777,216 elements.  The ring indexed in numpy."""
    cap, head, n, stride, F = 100003, 777, 1200, 7, 14003
    assert F * n > 65536 * 256
    ring = np.random.default_rng(5).standard_normal(cap)
    r_d = vb.to_device(ring)
    out = None
    try:
        vb.sync()
        t0 = time.perf_counter()
        out = vb.ring_frames(r_d, head, F, n, stride)
        vb.sync()
        dt = time.perf_counter() - t0
        got = out.numpy()
    finally:
        r_d.free()
        if out is not None:
            out.free()
    _note("ring-frames", F, None, None, ["ring_frames_kernel"], dt, elements=F * n)
    idx = (head + np.arange(F)[:, None] * stride + np.arange(n)[None, :]) % cap
    _same("ring-frames", "frames", got, ring[idx])


def test_f32_wide_past_the_capped_grids(vb, pattern):
    """vbx_autocorrelate_f32_wide at 512 samples and 512 lags on 32,803 frames: widen_frames_kernel and narrow_kernel (65,536 blocks each)
    both past 16,777,216 elements.  Against the f64 entry point on the widened frames, rounded once (tests/test_gpu_f32.py)."""
    n, hop, F = 512, 64, 32803
    assert F * n > 65536 * 256
    x32 = pf.tiled(pattern.astype(np.float32), pf.samples_needed(F, hop, n))
    w32 = np.hanning(n).astype(np.float32)
    x_d, w_d = vb.to_device(x32, np.float32), vb.to_device(w32, np.float32)
    out_d = _canary(vb, np.float32, F + K, n)
    try:
        dt = _timed(vb, lambda: vb._check(vb.L.vbx_autocorrelate_f32_wide(vb.ctx, x_d.ptr, F, n, hop, w_d.ptr, n, out_d.ptr)))
        got = out_d.numpy()
        # (which kernels such a call launches, from a small one)
        assert {"widen_frames", "narrow"} <= _profiled(vb, lambda: vb._check(vb.L.vbx_autocorrelate_f32_wide(vb.ctx, x_d.ptr, 64, n, hop, w_d.ptr, n, out_d.ptr)))
    finally:
        for a in (x_d, w_d, out_d):
            a.free()
    _note("f32-wide-autocorrelate", F, None, None, ["widen_frames_kernel", "narrow_kernel"], dt, elements=F * n)
    assert la.unwritten(got[F:]).shape[0] == K * n and not la.unwritten(got[:F]).size
    # the windowed product rounded to f32 first, as the reference's Windower<f32> produces it, then widened
    frames = np.lib.stride_tricks.sliding_window_view(x32, n)[::hop][:F]
    wide = (frames * w32[None, :]).astype(np.float32).astype(np.float64)
    want = vb.autocorrelate(wide, n)
    pa.rounded_once(got[:F], want, what="f32-wide-autocorrelate")


def _profiled(vb, fn):
    vb.profile_reset(); vb.profile(True)
    try:
        fn()
        return set(vb.profile_report())
    finally:
        vb.profile(False)


def test_synth_speech_past_the_capped_grid(vb, pkg):
    """synth_kernel: 16,384 blocks -- a second trip from 4,194,304 samples.  A sample is a function of its index alone: the long call
    equals short calls at the same offsets, bit for bit."""
    n = 16384 * 256 + 1003
    held = {}
    dt = _timed(vb, lambda: held.update(d=vb.synth_speech(n, sample_offset=OFFSET)))
    d = held["d"]
    got = d.numpy()
    d.free()
    for at in (0, 16384 * 256 - 500, n - 1000):
        s = vb.synth_speech(1000, sample_offset=OFFSET + at)
        _same("synth", f"samples from {at}", got[at:at + 1000], s.numpy())
        s.free()
    _note("synth-speech", n, None, None, ["synth_kernel"], dt)


def test_f32_to_f64_past_the_capped_grid(vb):
    """f32_to_f64_kernel: 8,192 blocks, two samples a thread -- a second trip from 4,194,304 samples; every element against numpy's cast."""
    n = 4194304 + 3
    x = np.random.default_rng(32).standard_normal(n).astype(np.float32)
    out_d = _canary(vb, np.float64, n + K)
    x_d = vb.to_device(x, np.float32)
    try:
        dt = _timed(vb, lambda: vb._check(vb.L.vbx_f32_to_f64(vb.ctx, x_d.ptr, n, out_d.ptr)))
        got = out_d.numpy()
    finally:
        x_d.free(); out_d.free()
    _note("f32-to-f64", n, None, None, ["f32_to_f64_kernel"], dt)
    assert n // 2 > 8192 * 256 and la.unwritten(got[n:]).shape[0] == K
    _same("f32-to-f64", "samples", got[:n], x.astype(np.float64))


UNPACK_PCM16, UNPACK_F64 = 1, 5


@pytest.mark.parametrize("fmt,group,dtype", [(UNPACK_PCM16, 8, np.int16), (UNPACK_F64, 2, np.float64)], ids=["pcm16", "f64"])
def test_unpack_samples_past_the_capped_grid(vb, fmt, group, dtype):
    """unpack_kernel: 8,192 blocks of 256 lanes, `group` samples a lane (vbx_reader.hpp) -- a second trip from 2,097,152 groups.  Channel 1
    of a stereo source, every element against numpy, the odd tail behind the groups included."""
    n = 8192 * 256 * group + group + 3
    rng = np.random.default_rng(fmt)
    src = (rng.integers(-32768, 32768, 2 * n).astype(np.int16) if fmt == UNPACK_PCM16 else rng.standard_normal(2 * n)).reshape(n, 2)
    s_d = vb.to_device(src.reshape(-1).view(np.uint8), np.uint8)
    out_d = _canary(vb, dtype, n + K)
    try:
        dt = _timed(vb, lambda: vb._check(vb.L.vbx_unpack_samples(vb.ctx, s_d.ptr, n, fmt, 2, 1, out_d.ptr)))
        got = out_d.numpy()
    finally:
        s_d.free(); out_d.free()
    name = f"unpack-samples-{np.dtype(dtype).name}"
    _note(name, n, None, None, ["unpack_kernel"], dt)
    assert la.unwritten(got[n:]).shape[0] == K
    _same(name, "channel 1", got[:n], np.ascontiguousarray(src[:, 1]))


@pytest.mark.parametrize("skew", [0, 2], ids=["tiled", "by-element"])
def test_unpack_channels_past_the_capped_grids(vb, skew):
    """vbx_unpack_channels on 16-bit stereo.  An aligned source goes through unpack_all_tiled_kernel, 2,048 blocks over tiles of 2,048
    sample frames: a second trip from 4,194,304 sample frames.  A source 2 bytes off a dword goes through unpack_all_elem_kernel, 8,192
    blocks of 256 lanes over frames * channels: a second trip from 1,048,576 sample frames.  Both planes against numpy."""
    n = (2048 * 2048 + 2048 + 5) if skew == 0 else (8192 * 256 // 2 + 5)
    src = np.random.default_rng(skew).integers(-32768, 32768, 2 * n).astype(np.int16).reshape(n, 2)
    raw = np.concatenate([np.zeros(skew, np.uint8), src.reshape(-1).view(np.uint8)])
    s_d = vb.to_device(raw, np.uint8)
    ld = (n + 127) // 128 * 128
    out_d = _canary(vb, np.int16, 2 * ld + K)
    sel = np.array([1, 0], dtype=np.int32)
    try:
        dt = _timed(vb, lambda: vb._check(vb.L.vbx_unpack_channels(vb.ctx, s_d.ptr + skew, n, UNPACK_PCM16, 2, sel.ctypes.data, 2, out_d.ptr, ld)))
        got = out_d.numpy()
    finally:
        s_d.free(); out_d.free()
    name = "unpack-channels-" + ("tiled" if skew == 0 else "by-element")
    _note(name, n, None, None, ["unpack_all_tiled_kernel" if skew == 0 else "unpack_all_elem_kernel"], dt)
    for k, c in enumerate((1, 0)):
        _same(name, f"plane {k}", got[k * ld:k * ld + n], np.ascontiguousarray(src[:, c]))
        assert la.unwritten(got[k * ld + n:(k + 1) * ld]).shape[0] == ld - n        # the padding between the planes
    assert la.unwritten(got[2 * ld:]).shape[0] == K


@pytest.mark.parametrize("n,env,form", [(700, {}, 4), (1200, {"VBX_MFCC_DFT2": "1"}, 5)], ids=["mfma", "dft2"])
def test_mfcc_kernels_past_their_block_caps(vb, pkg, oracle, pattern, n, env, form):
    """The matrix-core and the two-stage DFT kernels of vbx_mfcc_f64 load their tables once per block and stride over the frames: at most
    8 (16) blocks per CU of up to 8 wavefronts, a frame per wavefront.  The library has no probe for the grid: 70,003 frames exceed
    8 * 16 * the device's CUs, the most frames either grid can hold in one trip (asserted on the CU count the library reports); the
    period comparer holds every row, the first period's rows equal a call on them alone, and four of them meet the oracle."""
    F, name = 70003, f"mfcc-form{form}-{n}"
    ctx = _ctx(pkg, env) if env else vb
    try:
        cus = ctx.device_info()[1]
        assert F > 8 * 16 * cus, (F, cus)
        host = pf.tiled(pattern * 40.0, pf.samples_needed(F, HOP, n))              # (every filter's energy well above the log10 clamp)
        x_d = ctx.to_device(host)
        han = ctx.window(pkg.WINDOW_HANNING, n)
        out = (_canary(ctx, np.float64, F + K, 13), _canary(ctx, np.int32, F + K))
        dt = _timed(ctx, lambda: ctx.mfcc(x_d, 13, (100.0, 8000.0), SR, frame_len=n, stride=HOP, n_frames=F, window=han, out=out))
        assert int(ctx.L.vbx_internal_last_mfcc_form(ctx.ctx)) == form
        m, st = out[0].numpy(), out[1].numpy()
        rm, rst = ctx.mfcc(x_d, 13, (100.0, 8000.0), SR, frame_len=n, stride=HOP, n_frames=K, window=han)
        for a in out + (x_d,):
            a.free()
    finally:
        if env:
            ctx.close()
    _note(name, F, None, None, ["mfcc_mfma_kernel" if form == 4 else "mfcc_dft2_kernel"], dt, compute_units=cus)
    per = F                                                                         # (no host loop: one launch; a failure's message names the row alone)
    pf.assert_periodic(name, "mfcc", m, F, K, per)
    pf.assert_periodic(name, "status", st, F, K, per)
    _same(name, "mfcc[:211]", m[:K], rm)
    _same(name, "status[:211]", st[:K], rst)
    rows = [0, 70, 141, K - 1]
    w = oracle.window("hanning", n)
    pa.mfcc_rows(oracle, np.stack([host[f * HOP:f * HOP + n] * w for f in rows]), 13, 100.0, 8000.0, SR, m[rows], st[rows], what=name)


def test_host_chunk_rows_past_the_capped_grid(vb, pkg, pattern):
    """host_rows_kernel (vbx_analyze_host: a chunk's own rows into the caller's records): 8,192 blocks -- a second trip from 2,097,152 record
    entries, 58,255 frames of 36 columns.  Chunks of 60,011 frames of a 16-bit recording, two whole ones and a short one; every record
    and status against the resident call on the same samples, bit for bit."""
    N, H, chunk = 1200, 480, 60011
    F = 2 * chunk + 1003
    pcm = np.round(pf.tiled(pattern, pf.samples_needed(F, H, N)) * (0.9 * 32767.0)).astype(np.int16)
    params = pkg.AnalysisParams.make(SR, est_init=_est0(pkg))
    width = int(vb.L.vbx_record_doubles(C.byref(params)))
    assert width == 36 and chunk * width > 8192 * 256
    got = {}
    t0 = time.perf_counter()
    names = _profiled(vb, lambda: got.update(host=vb.analyze_host(pcm, params, None, None, chunk_frames=chunk, frame_len=N, stride=H, channel=0)))
    dt = time.perf_counter() - t0
    assert "host_rows" in names, sorted(names)
    want = vb.analyze_frames_ex_pcm16(pcm, params, None, None, frame_len=N, stride=H, n_frames=F)
    _note("host-chunk-rows", F, None, None, ["host_rows_kernel"], dt, chunk_frames=chunk)
    assert got["host"][0].shape[0] == F
    _same("host-chunk-rows", "records", got["host"][0][:, :width], want[0][:, :width])
    _same("host-chunk-rows", "status3", got["host"][1], want[1])


# ---- 6. what one push, tick or group holds: the ingest and row-copy kernels of sessions, pools and clip batches ---------------------------

N_LIVE, H_LIVE = 1200, 480


def _live_params(pkg):
    return pkg.AnalysisParams.make(SR, est_init=_est0(pkg))


def _same_rows(name, got, want, width):
    assert got[0].shape[0] == want[0].shape[0], (name, got[0].shape, want[0].shape)
    _same(name, "records", got[0][:, :width], want[0][:, :width])
    _same(name, "status3", got[1], want[1])


def test_session_push_past_the_capped_grids(vb, pkg, pattern):
    """One push of a 16-bit session that completes 60,011 frames from 28.8 M samples: session_ingest_kernel (8,192 blocks, 8 samples a
    lane: a second trip from 16,777,216 samples) and session_deliver_kernel (8,192 blocks: from 58,255 rows of 36 columns).  A second,
    small push follows it from the carried tail.  The pushes' rows together against the resident call on the whole signal, bit for bit."""
    F1 = 60011
    n1, n2 = pf.samples_needed(F1, H_LIVE, N_LIVE), 5003
    pcm = np.round(pf.tiled(pattern, n1 + n2) * (0.9 * 32767.0)).astype(np.int16)
    params = _live_params(pkg)
    got = {}
    with vb.session(params, format=pkg.SAMPLE_PCM16, frame_len=N_LIVE, stride=H_LIVE, max_block=n1) as sess:
        width = sess.rec
        assert n1 // 8 > 8192 * 256 and F1 * width > 8192 * 256
        t0 = time.perf_counter()
        names = _profiled(vb, lambda: got.update(a=sess.push(pcm[:n1])))
        dt = time.perf_counter() - t0
        got["b"] = sess.push(pcm[n1:])
    assert {"session_ingest_pcm16", "session_deliver"} <= names, sorted(names)
    F = pkg.frame_count(pcm.size, N_LIVE, H_LIVE)
    assert got["a"][0].shape[0] == F1 and got["b"][0].shape[0] == F - F1 > 0
    want = vb.analyze_frames_ex_pcm16(pcm, params, None, None, frame_len=N_LIVE, stride=H_LIVE, n_frames=F)
    _note("session-push", F, None, None, ["session_ingest_kernel", "session_deliver_kernel"], dt, frames_of_the_large_push=F1)
    both = (np.concatenate([got["a"][0], got["b"][0]]), np.concatenate([got["a"][1], got["b"][1]], axis=1))
    _same_rows("session-push", both, want, width)


def test_session_channels_push_past_the_capped_grids(vb, pkg, pattern):
    """One push of a 16-bit stereo session, both channels: 4.3 M sample frames complete 8,956 frames a channel.  session_ingest_all_kernel
    strides over 2,099 tiles of 2,048 sample frames with 2,048 blocks, session_deliver_all_kernel over 8,956 rows of 36 columns with 1,024
    blocks a channel (a second trip from 7,282 rows).  Each channel's rows against the resident call on that channel, bit for bit."""
    n = 4300003
    a = np.round(pf.tiled(pattern, n) * (0.9 * 32767.0)).astype(np.int16)
    b = np.round(pf.tiled(np.roll(pattern, 5000)[::-1], n) * (0.7 * 32767.0)).astype(np.int16)
    stereo = np.ascontiguousarray(np.stack([a, b], axis=1))
    params = _live_params(pkg)
    got = {}
    with vb.session_channels(params, format=pkg.SAMPLE_PCM16, channels=2, select=[1, 0], frame_len=N_LIVE, stride=H_LIVE, max_block=n) as sess:
        width = sess.rec
        F = pkg.frame_count(n, N_LIVE, H_LIVE)
        assert n // 2048 > 2048 and F * width > 1024 * 256
        t0 = time.perf_counter()
        names = _profiled(vb, lambda: got.update(rows=sess.push(stereo)))
        dt = time.perf_counter() - t0
    assert {"session_ingest_all_pcm16", "session_deliver_all"} <= names, sorted(names)
    _note("session-channels-push", F, None, None, ["session_ingest_all_kernel", "session_deliver_all_kernel"], dt, channels=2)
    for k, chan in enumerate((b, a)):
        want = vb.analyze_frames_ex_pcm16(chan, params, None, None, frame_len=N_LIVE, stride=H_LIVE, n_frames=F)
        _same_rows(f"session-channels-push channel {1 - k}", got["rows"][k], want, width)


def _three_signals(pattern, lengths):
    return [pf.tiled(np.roll(pattern, 3001 * i) * (0.9 - 0.2 * i), n) for i, n in enumerate(lengths)]


def test_pool_tick_past_the_capped_grids(vb, pkg, pattern):
    """One tick of a pool of f64 streams with three entries, 16.95 M samples and 35,306 rows together: pool_ingest_kernel (8,192 blocks
    over tiles of 1,024 groups of 2 samples: a second trip from 16,777,216 samples) and pool_deliver_kernel (2,048 blocks over 18 column
    pairs a row: from 29,128 rows).  Each slot's rows against the resident call on its block, bit for bit."""
    lengths = [8500003, 8400001, 50007]
    blocks = _three_signals(pattern, lengths)
    params = _live_params(pkg)
    got = {}
    with vb.pool(params, format=pkg.SAMPLE_F64, frame_len=N_LIVE, stride=H_LIVE, max_streams=4, max_block=max(lengths), max_tick=sum(lengths)) as pool:
        width = pool.rec
        t0 = time.perf_counter()
        names = _profiled(vb, lambda: got.update(tick=pool.push([(2, blocks[0]), (0, blocks[1]), (3, blocks[2])])))
        dt = time.perf_counter() - t0
    assert {"pool_ingest_f64", "pool_deliver"} <= names, sorted(names)
    rows, rec, st = got["tick"][:3]
    total = int(rows[:, 1].sum())
    assert sum(lengths) // 2 > 8192 * 256 * 4 and total * (width // 2) > 2048 * 256 and rec.shape[0] == total
    _note("pool-tick", total, None, None, ["pool_ingest_kernel", "pool_deliver_kernel"], dt, entries=3)
    for i, x in enumerate(blocks):
        r0, nr = int(rows[i, 0]), int(rows[i, 1])
        assert nr == pkg.frame_count(x.size, N_LIVE, H_LIVE)
        want = vb.analyze_frames_ex(x, params, None, None, frame_len=N_LIVE, stride=H_LIVE, n_frames=nr)
        _same_rows(f"pool-tick entry {i}", (rec[r0:r0 + nr], st[:, r0:r0 + nr]), want, width)


def test_clip_group_past_the_capped_grids(vb, pkg, pattern):
    """vbx_analyze_clips on three f64 clips that fall into ONE group (35,306 frames, below the default group of 69,905 at this hop):
    clips_pack_kernel (8,192 blocks over tiles of 1,024 groups of 2 samples: a second trip from 16,777,216 samples) and
    clips_deliver_kernel (2,048 blocks: from 29,128 rows).  Each clip's rows against the resident call on that clip alone, bit for bit."""
    lengths = [8500003, 8400001, 50007]
    clips = _three_signals(pattern, lengths)
    params = _live_params(pkg)
    width = int(vb.L.vbx_record_doubles(C.byref(params)))
    plan, total, groups = pkg.clips_plan(lengths, N_LIVE, H_LIVE)
    assert groups == 1 and sum(lengths) // 2 > 8192 * 256 * 4 and total * (width // 2) > 2048 * 256
    d = [vb.to_device(x) for x in clips]
    got = {}
    try:
        t0 = time.perf_counter()
        names = _profiled(vb, lambda: got.update(all=vb.analyze_clips(d, params=params, frame_len=N_LIVE, stride=H_LIVE)))
        dt = time.perf_counter() - t0
    finally:
        for a in d:
            a.free()
    assert {"clips_pack_f64", "clips_deliver"} <= names, sorted(names)
    rec, st = got["all"][:2]
    _note("clip-group", total, None, None, ["clips_pack_kernel", "clips_deliver_kernel"], dt, clips=3)
    for i, x in enumerate(clips):
        r0, nr = int(plan[i, 0]), int(plan[i, 1])
        want = vb.analyze_frames_ex(x, params, None, None, frame_len=N_LIVE, stride=H_LIVE, n_frames=nr)
        _same_rows(f"clip-group clip {i}", (rec[r0:r0 + nr], st[:, r0:r0 + nr]), want, width)


def test_zz_batch_seams_report():
    """Runs last in this file: every case's F, batching (from the probe), capped grids crossed and wall seconds, kept as a file when
    VBX_TEST_REPORT_DIR names a directory; profiles/batch_seams/report.json is the committed copy."""
    cases = REPORT["cases"]
    looped = [c for c in cases.values() if c["batches"] is not None]
    assert all(c["batches"] >= 2 and c["frames_per_batch"] % K != 0 for c in looped)
    REPORT["period_frames"], REPORT["hop"] = K, HOP
    out = os.environ.get("VBX_TEST_REPORT_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "batch_seams_report.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)
