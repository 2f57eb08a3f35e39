"""vbx_pitch_path_shard_begin_f64 / _enter / _finish and vbx_pitch_path_segment_peaks_f64 on the device: one device plays the
ranks, ONE CONTEXT PER PLAYED RANK (enter and finish need each rank's begin alive).  Every comparison is against
vbx_pitch_path_f64 on the whole recording in the same process: out_path as int64 views, out_index for equality."""
import ctypes as C

import numpy as np
import pytest

import pitch_path_shard_model as S

pytestmark = pytest.mark.gpu

INVALID = -1              # VBX_E_INVALID


def _random_lists(rng, F, kmax, zero_frac=0.1):               # as tests/test_gpu_pitch_path.py
    f = rng.uniform(60.0, 650.0, (F, kmax))
    f[rng.uniform(size=(F, kmax)) < zero_frac] = 0.0
    a = rng.uniform(0.0, 1.0, (F, kmax))
    cand = np.stack([f, a], axis=-1)
    count = rng.integers(0, kmax + 3, F).astype(np.int32)
    status = np.where(rng.uniform(size=F) < 0.03, rng.integers(1, 5, F), 0).astype(np.int32)
    lp = rng.uniform(0.0, 1.0, F) ** 3
    return cand, count, status, lp


@pytest.fixture(scope="module")
def ranks(pkg):
    """Eight contexts on device 0, shared by every test of the module."""
    ctxs = [pkg.VoxBox(0) for _ in range(8)]
    yield ctxs
    for c in ctxs:
        c.close()


def _plans(pkg, F, world, seg):
    out = []
    for r in range(world):
        pl = pkg.shard_plan(F, world, r, seg)
        out.append(dict(lo=pl.lo, hi=pl.hi, warm=pl.warm, continues_prev=pl.continues_prev, continues_next=pl.continues_next))
    return out


def _global_peaks(pkg, ranks, plans, lsegs, lp_dev, seg, F):
    """P of every local segment of every rank: vbx_pitch_path_segment_peaks_f64 per rank, then the host max (NaN ignored) over
    the ranks that share an utterance."""
    g = np.array([0], np.int64) if seg is None else np.asarray(seg, np.int64)
    peak = np.full(g.size, np.nan)
    ids = []
    for r, pl in enumerate(plans):
        a = pl["lo"] - pl["warm"]
        local = ranks[r].pitch_path_segment_peaks(lp_dev[r], pl["hi"] - a, lsegs[r])
        u = np.searchsorted(g, a + lsegs[r], side="right") - 1          # the whole recording's utterance of each local segment
        for j, uid in enumerate(u):
            if (lsegs[r][j + 1] if j + 1 < lsegs[r].size else pl["hi"] - a) > lsegs[r][j]:
                peak[uid] = np.fmax(peak[uid], local[j])
        ids.append(u)
    return [peak[u] for u in ids]


def _sharded(pkg, ranks, cand, count, status, lp, seg, kmax, world, plans=None, lsegs=None, **kw):
    """The protocol with one context per rank.  Returns (path [F, 2], index [F], chunks redone by enter per rank)."""
    F = cand.shape[0]
    params = pkg.PitchPathParams.make(**kw)
    seg_a = None if seg is None else np.asarray(seg, np.int64)
    plans = plans if plans is not None else _plans(pkg, F, world, seg_a)
    if lsegs is None:
        lsegs = [pkg.shard.plan_local_segments(pl, seg_a) for pl in plans]
    dev, keep = [], []
    for r, pl in enumerate(plans):
        a, b = pl["lo"] - pl["warm"], pl["hi"]
        vb = ranks[r]
        d = dict(cand=vb.to_device(np.ascontiguousarray(cand[a:b])), count=vb.to_device(np.ascontiguousarray(count[a:b])),
                 status=None if status is None else vb.to_device(np.ascontiguousarray(status[a:b])),
                 lp=None if lp is None else vb.to_device(np.ascontiguousarray(lp[a:b])),
                 path=vb.to_device(np.full((b - a, 2), -7.0)), index=vb.to_device(np.full(b - a, -7, np.int32)),
                 state=vb.empty(64), back=vb.empty(64, np.int32), changed=vb.empty(1, np.int32), end=vb.empty(1, np.int32))
        dev.append(d)
    peaks = [None] * world
    if lp is not None and params.silence_threshold != 0.0:
        pk = _global_peaks(pkg, ranks, plans, lsegs, [d["lp"] for d in dev], seg_a, F)
        peaks = [ranks[r].to_device(np.ascontiguousarray(pk[r])) for r in range(world)]
        keep += peaks
    try:
        for r, pl in enumerate(plans):                          # 1. begin, any order
            d = dev[r]
            ranks[r].pitch_path_shard_begin(d["cand"], d["count"], d["status"], pl["hi"] - pl["lo"] + pl["warm"], kmax, d["lp"], peaks[r],
                                            lsegs[r], params, pl["warm"], pl["continues_prev"], pl["continues_next"])

        def enter(r, state_in):                                 # 2. enter, in rank order (the previous context's stream is drained)
            d = dev[r]
            if r > 0:
                ranks[r - 1].sync()
            ranks[r].pitch_path_shard_enter(None if state_in is None else dev[r - 1]["state"], d["state"], d["back"], d["changed"])
            return d["state"], d["back"].numpy(), int(d["changed"].numpy()[0])

        def finish(r, end):                                     # 4. finish, any order
            d = dev[r]
            if end is not None:
                ranks[r].L.vbx_memcpy_h2d(ranks[r].ctx, d["end"].ptr, np.array([end], np.int32).ctypes.data, 4)
            ranks[r].pitch_path_shard_finish(None if end is None else d["end"], d["path"], 2, d["index"])
            p, i = d["path"].numpy(), d["index"].numpy()
            w = plans[r]["warm"]
            assert np.all(p[:w] == -7.0) and np.all(i[:w] == -7)           # rows [0, first) are not touched
            return p[w:], i[w:]

        rows, changed = pkg.shard.stitch_path(enter, finish, plans)
        redone = [ranks[r].last_path_chunks_redone() for r in range(world)]
        assert all(a >= b for a, b in zip(redone, changed))    # the running count: begin's repairs plus enter's
        return np.concatenate([p for p, _ in rows]), np.concatenate([i for _, i in rows]), changed
    finally:
        for d in dev:
            for x in d.values():
                if x is not None:
                    x.free()
        for x in keep:
            x.free()


def _whole(vb, pkg, cand, count, status, lp, seg, **kw):
    return vb.pitch_path(cand, count, status, lp, seg_start=None if seg is None else np.asarray(seg, np.int64),
                         params=pkg.PitchPathParams.make(**kw))


def _same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.int64), want[0].view(np.int64))


# ---- (a) random lists -----------------------------------------------------------------------------------------------------------

FA = 6000
SEG_A = [0, 2500, 2530, 4000]         # a cut utterance that ends inside a shard, a 30-frame utterance, a cut on a start
_REF = {}                             # (kmax, one utterance) -> (lists, the whole call's result): computed once


def _case_a(vb, pkg, kmax, seg):
    key = (kmax, seg is None)
    if key not in _REF:
        lists = _random_lists(np.random.default_rng(3000 + kmax), FA, kmax)
        _REF[key] = (lists, _whole(vb, pkg, *lists, seg))
    return _REF[key]


@pytest.mark.parametrize("seg", [None, SEG_A], ids=["one_utterance", "four_utterances"])
@pytest.mark.parametrize("kmax,world", [(k, w) for k in (1, 3, 15) for w in (2, 3, 8)] + [(63, 3)])
def test_random_lists_shard_to_the_whole_call(vb, pkg, ranks, kmax, world, seg):
    (cand, count, status, lp), want = _case_a(vb, pkg, kmax, seg)
    got = _sharded(pkg, ranks, cand, count, status, lp, seg, kmax, world)
    _same(got, want)


def test_a_cut_within_the_warm_up_of_an_utterance_start(vb, pkg, ranks):
    """An utterance that starts 30 frames before a cut: the next rank's local frame 0 IS its start (no state crosses)."""
    seg = [0, 1970, 4100]                                       # world 3: cuts at 2000 and 4000
    (cand, count, status, lp), _ = _case_a(vb, pkg, 3, None)
    plans = _plans(pkg, FA, 3, np.asarray(seg, np.int64))
    assert plans[1]["warm"] == 30 and not plans[1]["continues_prev"] and plans[2]["continues_prev"]
    _same(_sharded(pkg, ranks, cand, count, status, lp, seg, 3, 3), _whole(vb, pkg, cand, count, status, lp, seg))


# ---- (b) the two streams ------------------------------------------------------------------------------------------------------------

def _unstitched(vb, pkg, cand, count, plans, **kw):
    """Plain vbx_pitch_path_f64 on each rank's own frames (warm-up included): today's sharded contour."""
    out = []
    for pl in plans:
        a = pl["lo"] - pl["warm"]
        out.append(_whole(vb, pkg, cand[a:pl["hi"]], count[a:pl["hi"]], None, None, None, **kw)[1][pl["warm"]:])
    return np.concatenate(out)


@pytest.mark.parametrize("chunk", [0, 7, 5000], ids=["chunk_default", "chunk_7", "chunk_whole"])      # (d)
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["late", "early"])
def test_the_two_streams(vb, pkg, ranks, name, world, chunk):
    F = 3000
    cand, count = S.stream(name, world, F)
    want = _whole(vb, pkg, cand, count, None, None, None, **S.STREAM_PARAMS)
    assert np.all(want[1] == 1)                                # the whole path is track 1 throughout
    plans = _plans(pkg, F, world, None)
    loose = _unstitched(vb, pkg, cand, count, plans, **S.STREAM_PARAMS)
    assert int(np.sum(loose != want[1])) >= 1000               # the model gives 1500 / 1000: this test cannot pass vacuously
    path, index, changed = _sharded(pkg, ranks, cand, count, None, None, None, 2, world, chunk_frames=chunk, **S.STREAM_PARAMS)
    _same((path, index), want)
    if name == "late":
        assert all(n > 0 for n in changed[1:]), changed        # every receiving rank's guess was wrong
    assert changed[0] == 0


# ---- (c) first on the receiving rank ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [1, 5, 64])
def test_late_with_a_short_warm_up(vb, pkg, ranks, first):
    F, cut = 3000, 1500
    cand, count = S.stream("late", 2, F)
    want = _whole(vb, pkg, cand, count, None, None, None, **S.STREAM_PARAMS)
    plans = [dict(lo=0, hi=cut, warm=0, continues_prev=0, continues_next=1), dict(lo=cut, hi=F, warm=first, continues_prev=1, continues_next=0)]
    lsegs = [np.array([0], np.int64)] * 2
    path, index, changed = _sharded(pkg, ranks, cand, count, None, None, None, 2, 2, plans=plans, lsegs=lsegs, **S.STREAM_PARAMS)
    _same((path, index), want)
    assert changed[1] > 0


# ---- (d) chunk_frames on one case of (a) --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [0, 7, FA])
def test_chunk_frames_do_not_matter(vb, pkg, ranks, chunk):
    (cand, count, status, lp), want = _case_a(vb, pkg, 3, SEG_A)
    assert _plans(pkg, FA, 3, np.asarray(SEG_A, np.int64))[1]["warm"] % 7                       # the cut is no multiple of the chunk
    _same(_sharded(pkg, ranks, cand, count, status, lp, SEG_A, 3, 3, chunk_frames=chunk), want)


# ---- (e) the frame loop -------------------------------------------------------------------------------------------------------------

def test_the_tracked_frame_loop_shards_to_the_whole_call(vb, pkg, ranks):
    N, H, SR, P, F, kmax, world = 1200, 480, 48000.0, 12, 6000, 4, 3
    est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=P, formant_order=P, est_init=est0, mfcc=(13, 100.0, 8000.0))
    track = pkg.PitchTrackParams.make(kmax=kmax)
    path_params = pkg.PitchPathParams.make(time_step=H / SR)
    REC = int(vb.L.vbx_record_doubles(params))
    audio = vb.synth_speech((F - 1) * H + N, sample_offset=7 * 48000)
    whole, st_whole = vb.analyze_frames_tracked(audio, params, track, frame_len=N, stride=H, n_frames=F)
    plans = _plans(pkg, F, world, None)
    one = np.array([0], np.int64)
    dev = []
    for r, pl in enumerate(plans):                              # analyse, with the lists requested
        c = ranks[r]
        a, n = pl["lo"] - pl["warm"], pl["hi"] - pl["lo"] + pl["warm"]
        d = dict(rec=c.empty((n, REC)), st3=c.empty((3, n), np.int32), cand=c.empty((n, kmax, 2)), count=c.empty(n, np.int32),
                 peak=c.empty(n), index=c.empty(n, np.int32), state=c.empty(64), back=c.empty(64, np.int32), changed=c.empty(1, np.int32),
                 end=c.empty(1, np.int32), n=n)
        c.analyze_frames_tracked(audio.ptr + a * H * 8, params, track, seg_start=one, frame_len=N, stride=H, n_frames=n, out=d["rec"],
                                 record_ld=REC, status=d["st3"], outputs=(d["cand"], d["count"], d["peak"], d["index"]))
        if pl["continues_prev"]:                                # the formant stitch
            ranks[r - 1].sync()
            prev = dev[r - 1]
            c.track_stitch(d["rec"].ptr + 2 * 8, n, REC, pl["warm"], n, prev["rec"].ptr + ((prev["n"] - 1) * REC + 2) * 8, None)
        c.sync()
        dev.append(d)
    # the lists and counts of the frames two ranks share are the same bits
    for r in range(1, world):
        w = plans[r]["warm"]
        assert w == 64
        assert np.array_equal(dev[r]["cand"].numpy()[:w].view(np.int64), dev[r - 1]["cand"].numpy()[-w:].view(np.int64))
        assert np.array_equal(dev[r]["count"].numpy()[:w], dev[r - 1]["count"].numpy()[-w:])
    pk = np.fmax.reduce([ranks[r].pitch_path_segment_peaks(dev[r]["peak"], dev[r]["n"]) for r in range(world)])
    peaks = [ranks[r].to_device(pk) for r in range(world)]
    for r, pl in enumerate(plans):
        d = dev[r]
        ranks[r].pitch_path_shard_begin(d["cand"], d["count"], d["st3"], d["n"], kmax, d["peak"], peaks[r], one, path_params,
                                        pl["warm"], pl["continues_prev"], pl["continues_next"])

    def enter(r, state_in):
        d = dev[r]
        if r > 0:
            ranks[r - 1].sync()
        ranks[r].pitch_path_shard_enter(None if state_in is None else dev[r - 1]["state"], d["state"], d["back"], d["changed"])
        return d["state"], d["back"].numpy(), int(d["changed"].numpy()[0])

    def finish(r, end):
        d = dev[r]
        if end is not None:
            ranks[r].L.vbx_memcpy_h2d(ranks[r].ctx, d["end"].ptr, np.array([end], np.int32).ctypes.data, 4)
        ranks[r].pitch_path_shard_finish(None if end is None else d["end"], d["rec"], REC, d["index"])
        w = plans[r]["warm"]
        return d["rec"].numpy()[w:], d["st3"].numpy()[:, w:]

    rows, changed = pkg.shard.stitch_path(enter, finish, plans)
    got = np.concatenate([a for a, _ in rows])
    assert np.array_equal(got.view(np.int64), whole[:, :REC].view(np.int64))
    assert np.array_equal(np.concatenate([s for _, s in rows], axis=1), st_whole)
    print("tracked frame loop, world 3: chunks redone by enter", changed)
    for d in dev:
        for x in d.values():
            if not isinstance(x, int):
                x.free()
    for x in peaks + [audio]:
        x.free()


# ---- (f) misuse ---------------------------------------------------------------------------------------------------------------------

def test_misuse_is_rejected_and_the_context_stays_usable(vb, pkg, ranks):
    c, L = ranks[0], ranks[0].L
    (cand, count, status, lp), want = _case_a(vb, pkg, 3, None)
    F, kmax, first = 2000, 3, 64
    d = [c.to_device(np.ascontiguousarray(a[:F])) for a in (cand, count, status, lp)]
    canary_p, canary_i = np.full((F, 2), -7.0), np.full(F, -7, np.int32)
    path, idx = c.to_device(canary_p), c.to_device(canary_i)
    state, back, end = c.to_device(np.full(64, -7.0)), c.to_device(np.full(64, -7, np.int32)), c.to_device(np.zeros(1, np.int32))
    p = pkg.PitchPathParams.make()

    def begin(first=first, prev=1, nxt=1, n=F):
        return L.vbx_pitch_path_shard_begin_f64(c.ctx, d[0].ptr, d[1].ptr, d[2].ptr, n, kmax, d[3].ptr, None, None, 0, C.byref(p),
                                                first, prev, nxt)

    def enter(state_in=state.ptr):
        return L.vbx_pitch_path_shard_enter_f64(c.ctx, state_in, state.ptr, back.ptr, None)

    def finish(end_state=end.ptr):
        return L.vbx_pitch_path_shard_finish_f64(c.ctx, end_state, path.ptr, 2, idx.ptr)

    def untouched():
        c.sync()
        return (np.all(path.numpy() == -7.0) and np.all(idx.numpy() == -7) and np.all(state.numpy() == -7.0)
                and np.all(back.numpy() == -7))

    c.frame_peak(np.zeros(4800), frame_len=1200, stride=480)   # no begin on this context since a frame-batch call
    assert enter() == INVALID and finish() == INVALID and untouched()
    assert begin(first=F + 1) == INVALID and begin(first=0, prev=1) == INVALID and begin(n=0) == INVALID
    assert enter() == INVALID and finish() == INVALID and untouched()           # a rejected begin leaves nothing to continue
    assert begin() == 0
    assert enter(state_in=None) == INVALID and untouched()     # continues_prev needs the state
    assert finish() == INVALID and untouched()                 # finish before enter
    c.pitch_path(cand[:100], count[:100], status[:100], lp[:100])       # another path call in between
    assert enter() == INVALID and finish() == INVALID and untouched()
    assert begin() == 0
    c.L.vbx_memcpy_h2d(c.ctx, state.ptr, np.full(64, -np.inf).ctypes.data, 512)
    assert enter() == 0
    assert finish(end_state=None) == INVALID                   # continues_next needs the end state
    c.sync()
    assert np.all(path.numpy() == -7.0) and np.all(idx.numpy() == -7)
    assert finish() == 0
    assert np.all(idx.numpy()[:first] == -7) and not np.any(idx.numpy()[first:] == -7)
    # the next valid calls are right: first = 0 without continues_prev is the plain call
    assert begin(first=0, prev=0, nxt=0) == 0 and enter(state_in=None) == 0 and finish(end_state=None) == 0
    ref = vb.pitch_path(cand[:F], count[:F], status[:F], lp[:F])
    _same((path.numpy(), idx.numpy()), ref)
    for x in d + [path, idx, state, back, end]:
        x.free()


# ---- (g) the profiler ------------------------------------------------------------------------------------------------------------------

def test_every_new_launch_is_profiled(vb, pkg, ranks):
    cand, count = S.stream("late", 2, 3000)
    lp = np.linspace(0.1, 1.0, 3000)
    for c in ranks[:2]:
        c.profile(True)
        c.profile_reset()
    try:
        _sharded(pkg, ranks, cand, count, None, lp, None, 2, 2)
        rep = ranks[1].profile_report()
        rep0 = ranks[0].profile_report()
    finally:
        for c in ranks[:2]:
            c.profile(False)
    for name in ("pitch_path_segment_peaks", "pitch_path_spec", "pitch_path_enter", "pitch_path_backtrack", "pitch_path_export",
                 "pitch_path_select", "pitch_path_write"):
        assert name in rep and rep[name][1] >= 1, (name, sorted(rep))
    assert "pitch_path_open_map" in rep0 and rep0["pitch_path_open_map"][1] >= 1, sorted(rep0)
