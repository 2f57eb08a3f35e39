"""vbx_pool_plan, the host arithmetic of one tick of a session pool, without a GPU: against a Python restatement of the header's rules
built on pkg.session_plan, over a few thousand random (consumed, utt_frame, n_new) tuples per frame shape -- 400/160, 1200/480,
200/80, 100/250 (stride > frame_len) and 1/1.  The invariants: every entry's plan is vbx_session_plan's, rows are prefix sums in
entry order, entries without a frame have frames 0 and plane_frame -1, regions do not overlap and lie less than one hop apart, the
call covers the last region exactly; and the carried tail never exceeds VBX_SHARD_WARM_FRAMES * stride + frame_len - 1 samples, over
single tuples and over long random sequences of pushes, marks and resets per stream.  NULL and size rejections."""
import ctypes as C

import numpy as np
import pytest

SHAPES = [(400, 160), (1200, 480), (200, 80), (100, 250), (1, 1)]
WARM = 64


def carry_bound(N, H):
    return WARM * H + N - 1


def restated(pkg, cons, utt, new, N, H):
    """the header's layout rule, entry by entry: ([(plan dict, row_start, n_rows, frames, plane_frame)], total_rows, call_frames)"""
    rows, row, nxt, call = [], 0, 0, 0
    for c, u, n in zip(cons, utt, new):
        p = pkg.session_plan(c, u, n, N, H).as_dict()
        nf = p["hi"] - p["lo"]
        if nf == 0:
            rows.append((p, row, 0, 0, -1))
            continue
        m = p["warm"] + nf
        span = (p["hi"] - 1) * H + N - p["read_from"]            # samples [read_from, (hi - 1) * stride + frame_len)
        assert span == (m - 1) * H + N
        rows.append((p, row, nf, m, nxt))
        call = nxt + m
        nxt += -(-span // H)
        row += nf
    return rows, row, call


def random_tuples(pkg, rng, N, H, n):
    """n tuples: consumed anywhere from 0 to far past the warm-up, utt_frame anywhere up to the frames consumed (and, often, near
    them), n_new from 0 over sub-hop and exact-hop sizes to many hops"""
    out = []
    for _ in range(n):
        kind = int(rng.integers(0, 4))
        c = int(rng.integers(0, N + 3 * H)) if kind == 0 else int(rng.integers(0, N + 300 * H))
        lo = pkg.frame_count(c, N, H)
        u = int(rng.integers(0, lo + 1)) if kind != 2 else max(0, lo - int(rng.integers(0, 70)))
        k = int(rng.integers(0, 6))
        n_new = [0, 1, H - 1 if H > 1 else 1, H, int(rng.integers(0, 3 * H + 8)), N + int(rng.integers(0, 90 * H))][k]
        out.append((c, u, n_new))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}/{h}" for n, h in SHAPES])
def test_the_plan_is_the_restated_plan(pkg, shape):
    N, H = shape
    rng = np.random.default_rng(7100 + N + H)
    seen = dict(no_frame=False, frames=False, continues=False, fresh=False, inside=False, trailing=False, empty=False)
    n_tuples = 0
    ticks = [[]] + [random_tuples(pkg, rng, N, H, int(rng.integers(1, 40))) for _ in range(150)]
    for tick in ticks:
        cons, utt, new = ([t[k] for t in tick] for k in range(3))
        rows, total, call = pkg.pool_plan(cons, utt, new, N, H)
        want, w_total, w_call = restated(pkg, cons, utt, new, N, H)
        assert (total, call) == (w_total, w_call) and len(rows) == len(tick)
        n_tuples += len(tick)
        prev_end = None
        for i, (r, (p, row_start, n_rows, frames, plane_frame)) in enumerate(zip(rows, want)):
            d = r.as_dict()
            assert d["plan"] == p and (d["row_start"], d["n_rows"], d["frames"], d["plane_frame"]) == (row_start, n_rows, frames, plane_frame), (tick, i)
            c, u, n = tick[i]
            # what is carried afterwards, and what this push reads of what was carried before, stays within the bound
            assert c + n - p["keep_from"] <= carry_bound(N, H)
            if n_rows:
                assert d["frames"] == p["warm"] + n_rows and d["plane_frame"] >= 0
                off, span = plane_frame * H, (frames - 1) * H + N
                assert p["read_from"] + span <= c + n                                        # the region ends inside the block
                if prev_end is not None:
                    assert prev_end <= off < prev_end + H                                    # regions do not overlap, the gap is under a hop
                else:
                    assert off == 0
                prev_end = off + span
                seen["frames"] = True
                seen["continues"] |= bool(p["continues_prev"])
                seen["fresh"] |= not p["continues_prev"]
                seen["inside"] |= p["read_from"] > c                                         # read_from inside the block (stride > frame_len)
            else:
                assert (d["frames"], d["plane_frame"]) == (0, -1)
                seen["no_frame"] = True
                seen["trailing"] |= all(w[2] == 0 for w in want[i:]) and any(w[2] for w in want[:i])
        if prev_end is not None:
            assert (call - 1) * H + N == prev_end                                            # the call's last frame ends where the last region ends
        else:
            assert call == 0 and total == 0
            seen["empty"] = True
    assert n_tuples >= 2000
    if H > N:
        assert seen["inside"]
    seen["inside"] = True
    assert all(seen.values()), seen


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}/{h}" for n, h in SHAPES])
def test_the_carried_tail_stays_within_its_bound_over_long_sequences(pkg, shape):
    """a stream pushed blocks of every kind, marked and reset at random: what it carries, and what a push reads of the carried
    tail, never exceeds the region a pool slot has"""
    N, H = shape
    rng = np.random.default_rng(7200 + N + H)
    worst = 0
    for _ in range(6):
        c = utt = keep = 0
        for _ in range(400):
            k = int(rng.integers(0, 8))
            n = [1, max(H - 1, 1), H, H + 1, 3 * H + 7, N + 79 * H, int(rng.integers(1, 2 * H + 2)), int(rng.integers(1, N + 5 * H))][k]
            (r,), _, _ = pkg.pool_plan([c], [utt], [n], N, H)
            p = r.plan
            if p.hi > p.lo:
                assert keep <= p.read_from, "the push reads before what the slot carries"
                assert c - min(p.read_from, c) <= carry_bound(N, H)
            assert keep <= p.keep_from <= c + n                                               # the tail only moves forward
            c, keep = c + n, p.keep_from
            worst = max(worst, c - keep)
            assert c - keep <= carry_bound(N, H)
            u = rng.random()
            if u < 0.05:
                utt = pkg.frame_count(c, N, H)                                               # vbx_pool_mark_utterance
            elif u < 0.07:
                c = utt = keep = 0                                                            # vbx_pool_reset_stream
    assert worst == carry_bound(N, H) or H > N or (N, H) == (1, 1), worst                     # the bound is reached, not merely respected


def test_bad_arguments(pkg):
    L = pkg.load_library()
    sz = C.c_size_t
    a, b, c = (sz * 3)(0, 1000, 5000), (sz * 3)(0, 0, 3), (sz * 3)(400, 50, 900)
    rows = (pkg.PoolPlanRow * 3)()
    total, call = sz(7), sz(7)
    assert L.vbx_pool_plan(a, b, c, 3, 400, 160, rows, C.byref(total), C.byref(call)) == 0 and (total.value, call.value) == (8, 42)
    assert L.vbx_pool_plan(a, b, c, 3, 400, 160, rows, None, None) == 0                      # the totals are optional
    assert L.vbx_pool_plan(None, None, None, 0, 400, 160, None, C.byref(total), C.byref(call)) == 0 and (total.value, call.value) == (0, 0)
    for bad in ((None, b, c, 3, 400, 160, rows), (a, None, c, 3, 400, 160, rows), (a, b, None, 3, 400, 160, rows), (a, b, c, 3, 400, 160, None),
                (a, b, c, 3, 0, 160, rows), (a, b, c, 3, 400, 0, rows), (a, b, c, 3, 400, (1 << 40) + 1, rows)):
        assert L.vbx_pool_plan(*bad, C.byref(total), C.byref(call)) == -1, bad
    # an utterance start beyond the frames consumed (vbx_session_plan refuses it), and nothing is written for a refused tick
    marker = (pkg.PoolPlanRow * 3)()
    for r in marker:
        r.row_start = -5
    assert L.vbx_pool_plan(a, (sz * 3)(0, 0, 99), c, 3, 400, 160, marker, None, None) == -1
    assert all(r.row_start == -5 for r in marker)
    # a call of more than 0x7fffffff frames
    assert L.vbx_pool_plan((sz * 1)(0), (sz * 1)(0), (sz * 1)(1 << 31), 1, 1, 1, rows, None, None) == -1
    assert L.vbx_pool_plan((sz * 1)(0), (sz * 1)(0), (sz * 1)((1 << 31) - 1), 1, 1, 1, rows, C.byref(total), None) == 0 and total.value == (1 << 31) - 1
    with pytest.raises(pkg.VoxBoxError):
        pkg.pool_plan([0], [5], [100], 400, 160)
    assert C.sizeof(pkg.PoolPlanRow) == 48 + 32 and pkg.PoolPlanRow.row_start.offset == 48
