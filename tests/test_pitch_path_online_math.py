"""The online pitch path's definition (tests/pitch_path_online_model.py) against the whole utterance's path
(tests/pitch_path_model.py): what is committed without a flag IS the whole path, whatever follows and however small the ring.
No GPU: this holds the definition, the GPU tests hold the kernel to it."""
import numpy as np
import pytest

import pitch_path_model as M
import pitch_path_online_model as O
from pitch_path_shard_model import early_stream, late_stream

F = 600
NOSIL = dict(M.DEFAULTS, silence_threshold=0.0)


def _random_lists(rng, F, kmax, zero_frac=0.1):
    """tests/test_gpu_pitch_path.py's generator: bad statuses, count 0 and counts above kmax included"""
    f = rng.uniform(60.0, 650.0, (F, kmax))
    f[rng.uniform(size=(F, kmax)) < zero_frac] = 0.0
    a = rng.uniform(0.0, 1.0, (F, kmax))
    cand = np.stack([f, a], axis=-1)
    count = rng.integers(0, kmax + 3, F).astype(np.int32)
    status = np.where(rng.uniform(size=F) < 0.03, rng.integers(1, 5, F), 0).astype(np.int32)
    lp = rng.uniform(0.0, 1.0, F) ** 3
    return cand, count, status, lp


def _whole(tab, marks=None):
    seg = None if not marks else np.asarray([0] + sorted(m for m in marks if 0 < m < tab["F"]), np.int64)
    return M.path_states(tab, seg)


def _check_exact_prefixes(res, whole):
    """the committed prefix after every T is the whole path's, and committed(T) is monotone"""
    c = res["committed"]
    assert np.all(np.diff(c) >= 0)
    assert np.all(c <= np.arange(c.size))
    done = ~res["forced"] & (res["states"] >= 0)
    assert np.array_equal(res["states"][done], whole[done])


@pytest.mark.parametrize("kmax", [1, 3, 15, 63])
def test_random_lists_commit_the_whole_path(kmax):
    rng = np.random.default_rng(4000 + kmax)
    cand, count, status, lp = _random_lists(rng, F, kmax)
    tab = M.frame_table(cand, count, status, None, None, NOSIL)
    whole = M.path_states(tab, None)
    res = O.run(tab, 64, marks=[F])
    assert res["max_pending_seen"] < 64, res["max_pending_seen"]          # below the cap: nothing can be forced ...
    assert not res["forced"].any()
    _check_exact_prefixes(res, whole)
    for T in range(F + 1):                                     # ... and the committed prefix after every T is the whole path's
        c = res["before_mark"][T]
        assert np.array_equal(res["states"][:c], whole[:c])
    assert res["committed"][F] == F                            # the flush gives the rest
    assert np.array_equal(res["states"], whole)
    # the same run without the flush commits the same states for what it commits
    res2 = O.run(tab, 64)
    c = res2["committed"][F]
    assert c == res["before_mark"][F] and np.array_equal(res2["states"][:c], whole[:c]) and np.all(res2["states"][c:] == -1)


@pytest.mark.parametrize("kmax", [1, 3, 15, 63])
def test_peak_ref_replaces_the_utterance_peak(kmax):
    rng = np.random.default_rng(4100 + kmax)
    cand, count, status, lp = _random_lists(rng, F, kmax)
    p = dict(M.DEFAULTS, silence_threshold=0.03)
    peak_ref = 0.8
    tab = O.online_table(cand, count, status, lp, peak_ref, p)
    # u recomputed from P = peak_ref by the resident model's own formula: local_peak with one more frame that holds peak_ref
    ref = M.frame_table(np.concatenate([cand, cand[:1]]), np.append(count, 0), np.append(status, 0),
                        np.append(np.minimum(lp, peak_ref), peak_ref), None, p)
    clipped = lp > peak_ref                                    # (frames above peak_ref: rho > 1 there, u = vt either way)
    assert np.array_equal(tab["u"][~clipped], ref["u"][:F][~clipped])
    assert np.all(tab["u"][clipped] == p["voicing_threshold"])
    assert np.any(tab["u"] > p["voicing_threshold"])           # the silence term is at work
    whole = M.path_states(tab, None)
    res = O.run(tab, 64, marks=[F])
    assert not res["forced"].any() and np.array_equal(res["states"], whole)


@pytest.mark.parametrize("name", ["late", "early"])
def test_two_track_streams_force_rows_at_the_cap(name):
    cand, count = (late_stream if name == "late" else early_stream)(F, 300)
    tab = M.frame_table(cand, count, None, None, None, NOSIL)
    whole = M.path_states(tab, None)
    mp = 16
    res = O.run(tab, mp, marks=[F])
    assert res["forced"].any()
    _check_exact_prefixes(res, whole)
    assert np.all(res["states"] >= 0)
    flushed = ~res["forced"]
    assert np.array_equal(res["states"][flushed], whole[flushed])
    # the forced positions: the traces never merge, so the ring fills after mp frames, 8 frames go, and again every 8 frames
    want = np.zeros(F, bool)
    com = 0
    for t in range(F):
        if t - com == mp:
            want[com:com + 8] = True
            com += 8
    assert np.array_equal(res["forced"], want)
    assert np.sum(flushed) == mp                               # the flush at the end commits a full ring
    assert res["max_pending_seen"] == mp


def test_mixed_stream_has_forced_and_exact_rows():
    rng = np.random.default_rng(4200)
    a = _random_lists(rng, 250, 2)
    b = _random_lists(rng, 250, 2)
    tc, tn = late_stream(100, 50)
    cand = np.concatenate([a[0], tc, b[0]])
    count = np.concatenate([a[1], tn, b[1]])
    status = np.concatenate([a[2], np.zeros(100, np.int32), b[2]])
    tab = M.frame_table(cand, count, status, None, None, NOSIL)
    whole = M.path_states(tab, None)
    res = O.run(tab, 32, marks=[F])
    assert res["forced"].any() and (~res["forced"]).sum() > 400
    assert np.all(res["forced"][:250 - 32] == 0) and np.all(res["forced"][350:] == 0)
    _check_exact_prefixes(res, whole)
    assert np.all(res["states"] >= 0)


def test_marks_equal_seg_start():
    rng = np.random.default_rng(4300)
    cand, count, status, lp = _random_lists(rng, F, 7)
    marks = [1, 2, 57, 300, 301, 599, F]
    tab = M.frame_table(cand, count, status, None, None, NOSIL)
    whole = _whole(tab, marks)
    res = O.run(tab, 64, marks=marks)
    assert not res["forced"].any()
    assert np.array_equal(res["states"], whole)
    for m in marks:                                            # a mark delivers the rest at once
        assert res["committed"][m] == m
    assert not np.array_equal(whole, M.path_states(tab, None))  # (the marks matter on this stream)


def test_commit_records_follow_the_schedule():
    rng = np.random.default_rng(4400)
    cand, count, status, lp = _random_lists(rng, 200, 3)
    tab = M.frame_table(cand, count, status, None, None, NOSIL)
    res = O.run(tab, 4, marks=[100, 200])
    for step in (1, 7, 200):
        pushes = [(T, T in (100, 200)) for T in sorted(set(list(range(step, 201, step)) + [100, 200]))]
        recs = O.commits(res, pushes)
        assert recs[0][0] == 0 and sum(r[1] for r in recs) == 200
        for (first, n, nf, pend), (T, _) in zip(recs, pushes):
            assert first + n + pend == T and 0 <= pend <= 4 and nf == res["forced"][first:first + n].sum()
    # a zero-frame push that carries the mark: the push before it reports what was decided, the mark the rest
    recs = O.commits(res, [(100, False), (100, True), (200, True)])
    assert recs[0][3] == 100 - res["before_mark"][100] and recs[1] == (int(res["before_mark"][100]), recs[0][3], 0, 0)
