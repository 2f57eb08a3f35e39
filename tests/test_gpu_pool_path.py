"""vbx_pool_path_bind on a real MI355X: every slot's live pitch contour from ONE more launch per tick (include/voxbox_hip.h, DESIGN.md
section 5m), against yardsticks that are never the new code: a BOUND one-channel vbx_session pushed the same blocks, marks and resets
(rows, indices, forced flags and commit records), the RESIDENT tracked call on a stream's whole recording, and vbx_analyze_clips
where hundreds of streams must be compared fast.  Nothing is compared with a tolerance: the arrays are canary-filled and compared on
integer views, and no case is left out of any comparison (share of cases skipped: 0).  Streams, schedules and ticks are
test_gpu_pool's (_streams, _sizes, _ticks, _open_pool where the form's kmax 4 is what the case wants), the session side is
test_gpu_session_path's (Run, MP).  References are computed once per key and never changed."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_pool as gp
import test_gpu_session_path as sp
from test_gpu_session import base  # noqa: F401  (the module's recording fixture)

pytestmark = pytest.mark.gpu

F, MP = sp.F, sp.MP
SMALL, NATIVE = gp.SMALL, gp.NATIVE
E_INVALID = -1
i32, i64, u8 = np.int32, np.int64, np.uint8
CANARY = 0xFFFFFFFFFFFFFFFF
_u64 = sp._u64
_SESS, _RES = {}, {}


# ---- the harness ------------------------------------------------------------------------------------------------------------------

class Bound:
    """the arrays a pool is bound to -- [n_slots * slot_rows] rows, n_slots commit records -- canary-filled before every tick"""

    def __init__(self, vb, n_slots, slot_rows, ld=2):
        self.vb, self.S, self.R, self.ld = vb, n_slots, slot_rows, ld
        tot = n_slots * slot_rows
        self.path, self.index, self.forced, self.commit = vb.empty((tot, ld)), vb.empty(tot, i32), vb.empty(tot, u8), vb.empty((n_slots, 4), i64)
        self.all = [self.path, self.index, self.forced, self.commit]
        self.clear()

    def clear(self):
        for d in self.all:
            self.vb._check(self.vb.L.vbx_memset(self.vb.ctx, d.ptr, 0xFF, d.nbytes))

    def bind(self, pool, peak_ref=1.0, mp=MP, **kw):
        return pool.bind_path(self.path.ptr, self.commit.ptr, peak_ref=peak_ref, max_pending=mp, path_ld=self.ld, slot_rows=self.R,
                              out_index=self.index.ptr, out_forced=self.forced.ptr, **kw)

    def take(self, visited):
        """{slot: (rows [n, 2], index, forced, commit)} of the visited slots; rows past n, the columns past 1 and everything of the
        other slots must still be the canary"""
        self.vb.sync()
        p, ix, fo, cm = (d.numpy() for d in self.all)
        out = {}
        for s in range(self.S):
            a = s * self.R
            if s not in visited:
                assert np.all(cm[s] == -1), ("the commit record of an unvisited slot was written", s, cm[s])
                n = 0
            else:
                n = int(cm[s, 1])
                assert 0 <= n <= self.R, (s, cm[s])
                out[s] = (p[a:a + n, :2].copy(), ix[a:a + n].copy(), fo[a:a + n].copy(), tuple(int(v) for v in cm[s]))
            assert np.all(_u64(p[a + n:a + self.R]) == CANARY) and np.all(_u64(p[a:a + n, 2:]) == CANARY), ("rows past n were written", s)
            assert np.all(ix[a + n:a + self.R] == -1) and np.all(fo[a + n:a + self.R] == 0xFF), ("rows past n were written", s)
        return out

    def free(self):
        for d in self.all:
            d.free()


class TickOut:
    """a tick's own outputs (records, status rows, lists of `cap` rows): what the path launch must not depend on"""

    def __init__(self, vb, pkg, kmax, cap):
        p = sp._params(pkg)
        self.vb, self.cap, self.kmax = vb, cap, kmax
        self.width = int(vb.L.vbx_record_doubles_ex(C.byref(p), None))
        self.ld = self.width + (self.width & 1)
        self.rec, self.st = vb.empty((cap, self.ld)), vb.empty((3, cap), i32)
        self.lists = [vb.empty((cap, kmax, 2)), vb.empty(cap, i32), vb.empty(cap)]
        self.all = [self.rec, self.st] + self.lists
        self.clear()

    def clear(self):
        for d in self.all:
            self.vb._check(self.vb.L.vbx_memset(self.vb.ctx, d.ptr, 0xFF, d.nbytes))

    def kw(self):
        return dict(out=self.rec.ptr, status=self.st.ptr, outputs=tuple(d.ptr for d in self.lists) + (None,), record_ld=self.ld, status_ld=self.cap)

    def free(self):
        for d in self.all:
            d.free()


def _pool(vb, pkg, shape, n, kmax, silence, max_block, max_tick=None):
    if kmax == gp.KMAX and silence == 0.03:                    # the tracked form of test_gpu_pool
        return gp._open_pool(vb, pkg, "pcm16", shape, "tracked", n, max_block, max_tick)
    return vb.pool(sp._params(pkg), None, sp._track(pkg, kmax, silence), format=1, frame_len=shape[0], stride=shape[1], max_streams=n,
                   max_block=max_block, max_tick=max_tick)


class Got:
    """one slot's contour as the ticks committed it, and its per-tick commit records"""

    def __init__(self):
        self.p, self.ix, self.fo, self.cm = [], [], [], []

    def add(self, t):
        self.p.append(t[0]); self.ix.append(t[1]); self.fo.append(t[2]); self.cm.append(t[3])

    def arrays(self):
        return (np.concatenate(self.p) if self.p else np.empty((0, 2)), np.concatenate(self.ix) if self.ix else np.empty(0, i32),
                np.concatenate(self.fo) if self.fo else np.empty(0, u8))


def _run_pool(vb, pool, bd, tk, streams, scheds, ticks, marks=None, final=True):
    """feeds the ticks (an utterance is marked wherever a stream's delivered frames reach one of its marks, as test_gpu_pool does);
    final: every slot is marked and an EMPTY tick fetches the tails.  Returns one Got per stream."""
    n = len(streams)
    got = [Got() for _ in range(n)]
    pos, nxt, done = [0] * n, [0] * n, [set() for _ in range(n)]
    for pick in ticks:
        entries = []
        for k in pick:
            lo = pool.info(k)[1]
            if marks and lo in marks.get(k, ()) and lo not in done[k]:
                done[k].add(lo)
                pool.mark_utterance(k)
            sz = scheds[k][nxt[k]]
            entries.append((k, streams[k][0][pos[k]:pos[k] + sz]))
            pos[k] += sz
            nxt[k] += 1
        bd.clear()
        rows, total = pool.push(entries, **tk.kw())
        assert total <= tk.cap
        out = bd.take(set(pick))
        for k in pick:
            got[k].add(out[k])
    if final:
        for k in range(n):
            pool.mark_utterance(k)
        bd.clear()
        rows, total = pool.push([], **tk.kw())
        assert total == 0 and rows.shape == (0, 2)
        out = bd.take(set(range(n)))
        for k in range(n):
            got[k].add(out[k])
    return got


def _merge(a, b):
    """a deferred mark's record and the push's behind it: `first` of the first, n and n_forced summed, `pending` of the last"""
    return (a[0], a[1] + b[1], a[2] + b[2], b[3])


def _session(vb, pkg, key, audio, shape, kmax, silence, sizes, marks=(), mp=MP, peak_ref=1.0, final=True):
    """a BOUND one-channel session on the same blocks and marks: (rows, index, forced, the commit records as the pool must report
    them -- a mark's record merged into the next push's, the final mark's on its own).  Computed once per key."""
    if key in _SESS:
        return _SESS[key]
    N, H = shape
    run = sp.Run(vb, pkg, kmax, len(sizes) + len(marks) + 2, mp + max(sizes) // H + 2)
    try:
        with sp._open(vb, pkg, "pcm16", 1, N, H, kmax, max(sizes), silence) as sess:
            pos, slot, done, kinds = 0, 0, set(), []
            for n in sizes:
                lo = sess.info()[1]
                if lo in marks and lo not in done:
                    done.add(lo)
                    run.bind(sess, slot, peak_ref, mp); slot += 1; kinds.append("m")
                    sess.mark_utterance()
                run.bind(sess, slot, peak_ref, mp); slot += 1; kinds.append("p")
                assert sess.push(audio[pos:pos + n], **run.push_args(lo)) is None
                pos += n
            if final:
                run.bind(sess, slot, peak_ref, mp); slot += 1; kinds.append("f")
                sess.mark_utterance()
            gp_, gi, gf, cm = run.contour(slot)
        want, held = [], None
        for kind, c in zip(kinds, cm):
            if kind == "m":
                held = c
            else:
                want.append(c if held is None else _merge(held, c))
                held = None
        _SESS[key] = (gp_, gi, gf, want)
    finally:
        run.free()
    return _SESS[key]


def _resident(vb, pkg, key, pcm, shape, kmax, frames, seg=None):
    if key not in _RES:
        _RES[key] = vb.analyze_frames_ex_pcm16(pcm, sp._params(pkg), None, sp._track(pkg, kmax, 0.0), seg_start=None if seg is None else np.asarray(seg, i64),
                                               frame_len=shape[0], stride=shape[1], n_frames=frames, lists=True)
    return _RES[key]


def _equal(label, got, want):
    a, wa = got.arrays(), want
    assert a[0].shape == wa[0].shape, (label, a[0].shape, wa[0].shape)
    x, y = _u64(a[0]), _u64(wa[0])
    assert np.array_equal(x, y), (label, "first differing rows", np.argwhere(x != y)[:4])
    assert np.array_equal(a[1], wa[1]), (label, "index")
    assert np.array_equal(a[2], wa[2]), (label, "forced")
    assert got.cm == wa[3], (label, "commit records", [(i, g, w) for i, (g, w) in enumerate(zip(got.cm, wa[3])) if g != w][:4])


# ---- 1. the pool against bound sessions and the resident call ----------------------------------------------------------------------

@pytest.mark.parametrize("silence", [0.0, 0.03])
@pytest.mark.parametrize("kmax", [4, 15])
@pytest.mark.parametrize("shape", [SMALL, NATIVE])
def test_the_pool_against_bound_sessions_and_the_resident_call(vb, pkg, base, shape, kmax, silence):
    N, H = shape
    n, T = 5, (F - 1) * H + N
    streams = gp._streams(base, "pcm16", shape, n)
    rng = np.random.default_rng(5000 + kmax)
    scheds = [gp._sizes(rng, N, H, T, big_first=k % 2 == 0) for k in range(n)]
    assert any(N + 79 * H in s for s in scheds)
    ticks = gp._ticks(rng, scheds)
    assert len(ticks[0]) == n and all(s[0] == 1 for s in scheds) and any(len(t) == 1 for t in ticks)
    reach = []                                                 # the frames each stream has delivered when one of its pushes begins
    for s in scheds:
        c, fr = 0, []
        for sz in s:
            fr.append(pkg.frame_count(c, N, H))
            c += sz
        reach.append(sorted(set(fr)))
    marks = {0: {reach[0][len(reach[0]) // 3], reach[0][2 * len(reach[0]) // 3]}, 1: {reach[1][len(reach[1]) // 2]}, 3: {0, reach[3][-3]}}
    assert len({tuple(sorted(m)) for m in marks.values()}) == 3
    mb = max(max(s) for s in scheds)
    R = pkg.pool_path_slot_rows(MP, mb, H)
    assert R == MP + -(-mb // H)
    bd, tk = Bound(vb, n, R), TickOut(vb, pkg, kmax, sum(max(s) for s in scheds) // H + n + 2)
    try:
        with _pool(vb, pkg, shape, n, kmax, silence, mb) as pool:
            assert bd.bind(pool) == R
            got = _run_pool(vb, pool, bd, tk, streams, scheds, ticks, marks)
            assert all(pool.info(k)[1] == F for k in range(n))
    finally:
        bd.free(); tk.free()
    contours = []
    for k in range(n):
        mk = tuple(sorted(marks.get(k, ())))
        label = f"{shape} kmax {kmax} silence {silence} stream {k}"
        want = _session(vb, pkg, ("t1", shape, kmax, silence, k), streams[k][0], shape, kmax, silence, scheds[k], mk)
        assert not want[2].any(), "the session reference forces no row at this cap"
        _equal(label + ": the bound session", got[k], want)
        p, ix, fo = got[k].arrays()
        assert p.shape == (F, 2) and sum(c[1] for c in got[k].cm) == F and got[k].cm[-1][3] == 0 and not fo.any()
        first = 0
        for c in got[k].cm:                                    # the records chain
            assert c[0] == first and c[2] == 0 and 0 <= c[3] <= MP, c
            first += c[1]
        if silence == 0.0:
            seg = [0] + [m for m in mk if m > 0] if mk else None
            res = _resident(vb, pkg, ("t1", shape, kmax, k, mk), streams[k][1], shape, kmax, F, seg)
            assert np.array_equal(_u64(p), _u64(res[0][:, :2])) and np.array_equal(ix, res[5]), label + ": the resident call"
        contours.append(_u64(p).tobytes())
    assert len(set(contours)) == n                             # a slot mix-up cannot pass


# ---- 2. forced rows --------------------------------------------------------------------------------------------------------------

def test_forced_rows(vb, pkg, base):
    shape, kmax, n, mp = SMALL, 15, 3, 3
    N, H = shape
    T = (F - 1) * H + N
    streams = gp._streams(base, "pcm16", shape, 5)[:n]
    rng = np.random.default_rng(5100)
    scheds = [gp._sizes(rng, N, H, T, big_first=k % 2 == 0) for k in range(n)]
    ticks = gp._ticks(rng, scheds)
    mb = max(max(s) for s in scheds)
    R = pkg.pool_path_slot_rows(mp, mb, H)
    bd, tk = Bound(vb, n, R), TickOut(vb, pkg, kmax, sum(max(s) for s in scheds) // H + n + 2)
    try:
        with _pool(vb, pkg, shape, n, kmax, 0.0, mb) as pool:
            bd.bind(pool, mp=mp)
            got = _run_pool(vb, pool, bd, tk, streams, scheds, ticks)
    finally:
        bd.free(); tk.free()
    forced = 0
    for k in range(n):
        want = _session(vb, pkg, ("t2", k), streams[k][0], shape, kmax, 0.0, scheds[k], mp=mp)
        forced += int(want[2].sum())
        _equal(f"forced, stream {k}", got[k], want)
    assert forced > 0, "the session reference forces rows: the case is not vacuous"


# ---- 3. the narrowest and widest lane groups -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kmax", [3, 63])
def test_the_narrowest_and_widest_lane_groups(vb, pkg, base, kmax):
    shape, n, frames = SMALL, 3, 60
    N, H = shape
    T = (frames - 1) * H + N
    streams = gp._streams(base, "pcm16", shape, n, frames)
    scheds = [[1, N + 20 * H, H - 1, 1] + [3 * H + 7] * 5, [N, H, H] + [7 * H + 3] * 4, [T]]
    for s in scheds:
        s.append(T - sum(s))
        if s[-1] == 0:
            s.pop()
        assert sum(s) == T and min(s) >= 1
    ticks = gp._ticks(np.random.default_rng(5200 + kmax), scheds)
    mb = T
    r1 = sorted(_reach(pkg, scheds[1], N, H))
    marks = {1: {r1[len(r1) // 2]}}                            # stream 1 is marked mid-call
    assert 0 < r1[len(r1) // 2] < frames
    R = pkg.pool_path_slot_rows(MP, mb, H)
    bd, tk = Bound(vb, n, R), TickOut(vb, pkg, kmax, 3 * frames)
    try:
        with _pool(vb, pkg, shape, n, kmax, 0.0, mb) as pool:
            bd.bind(pool)
            got = _run_pool(vb, pool, bd, tk, streams, scheds, ticks, marks)
    finally:
        bd.free(); tk.free()
    for k in range(n):
        mk = tuple(sorted(marks.get(k, ())))
        want = _session(vb, pkg, ("t3", kmax, k), streams[k][0], shape, kmax, 0.0, scheds[k], mk)
        _equal(f"kmax {kmax}, stream {k}", got[k], want)
        assert got[k].arrays()[0].shape == (frames, 2)


def _reach(pkg, sizes, N, H):
    c, fr = 0, set()
    for sz in sizes:
        fr.add(pkg.frame_count(c, N, H))
        c += sz
    return fr


# ---- 4. more than one commit tile -------------------------------------------------------------------------------------------------

def test_more_than_one_commit_tile(vb, pkg, base):
    """stream 0 in ONE block of 320 frames with max_pending 512: the final mark commits more than PP_TILE = 256 rows at once"""
    shape, kmax, frames, mp = SMALL, 4, 320, 512
    N, H = shape
    T = (frames - 1) * H + N
    streams = gp._streams(base, "pcm16", shape, 2, frames)
    scheds = [[T], [N] + [H] * (frames - 1)]
    ticks = [[0, 1]] + [[1]] * (frames - 1)
    R = pkg.pool_path_slot_rows(mp, T, H)
    bd, tk = Bound(vb, 2, R), TickOut(vb, pkg, kmax, frames + 4)
    try:
        with _pool(vb, pkg, shape, 2, kmax, 0.0, T) as pool:
            bd.bind(pool, mp=mp)
            got = _run_pool(vb, pool, bd, tk, streams, scheds, ticks)
    finally:
        bd.free(); tk.free()
    assert max(c[1] for c in got[0].cm) > 256
    for k in range(2):
        p, ix, fo = got[k].arrays()
        res = _resident(vb, pkg, ("t4", k), streams[k][1], shape, kmax, frames)
        assert p.shape == (frames, 2) and not fo.any() and got[k].cm[-1][3] == 0
        assert np.array_equal(_u64(p), _u64(res[0][:, :2])) and np.array_equal(ix, res[5]), k


# ---- 5. past the argument-table cap -------------------------------------------------------------------------------------------------

def test_past_the_argument_table_cap(vb, pkg, base):
    """130 streams (the multi-channel kernel's descriptors stop at 64), random ticks; every slot against vbx_analyze_clips (tracked)
    on the streams as clips, with the path the resident way (silence 0: the rows are the tracked call's columns 0-1 and index)"""
    shape, kmax, n, frames = SMALL, 4, 130, 40
    N, H = shape
    T = (frames - 1) * H + N
    streams = gp._streams(base, "pcm16", shape, n, frames)
    rng = np.random.default_rng(5400)
    menu = [1, H - 1, H, 3 * H + 7, 7 * H + 3, N + 9 * H]
    scheds = []
    for k in range(n):
        s = [1]
        while sum(s) < T:
            s.append(int(menu[int(rng.integers(0, len(menu)))]))
        s[-1] -= sum(s) - T
        if s[-1] == 0:
            s.pop()
        scheds.append(s)
    ticks = gp._ticks(rng, scheds)
    mb = N + 9 * H
    R = pkg.pool_path_slot_rows(MP, mb, H)
    track = sp._track(pkg, kmax, 0.0)
    bd, tk = Bound(vb, n, R), TickOut(vb, pkg, kmax, n * (mb // H + 2))
    try:
        with vb.pool(sp._params(pkg), None, track, format=1, frame_len=N, stride=H, max_streams=n, max_block=mb) as pool:
            bd.bind(pool)
            got = _run_pool(vb, pool, bd, tk, streams, scheds, ticks)
    finally:
        bd.free(); tk.free()
    clips = [vb.to_device(s[0], np.int16) for s in streams]
    try:
        res = vb.analyze_clips(clips, params=sp._params(pkg), track=track, frame_len=N, stride=H, lists=True)
    finally:
        for c in clips:
            c.free()
    assert res[0].shape[0] == n * frames
    seen = set()
    for k in range(n):
        p, ix, fo = got[k].arrays()
        a = k * frames
        assert p.shape == (frames, 2) and not fo.any(), k
        assert np.array_equal(_u64(p), _u64(res[0][a:a + frames, :2])) and np.array_equal(ix, res[5][a:a + frames]), k
        seen.add(_u64(p).tobytes())
    assert len(seen) > n // 2                                  # (the mix repeats a few short contours; most differ, so a shifted slot cannot pass)


# ---- 6. reset ------------------------------------------------------------------------------------------------------------------------

def test_reset(vb, pkg, base):
    """slot 1 is fed 50 frames of stream A and reset with frames pending: they are dropped, `first` restarts at 0 and its rows equal a
    fresh bound session's on stream B; slot 0, fed alongside, equals its own session.  Then: mark, empty tick, reset delivers the old
    call's tail first."""
    shape, kmax, frames = SMALL, 4, 60
    N, H = shape
    T = (frames - 1) * H + N
    streams = gp._streams(base, "pcm16", shape, 3, frames)
    a_audio, b_audio = streams[2][0], streams[1][0]
    first = N + 49 * H
    rest = [N + 9 * H, 5 * H, T - (N + 14 * H)]
    s0 = [first, 1000, T - first - 1000]
    R = pkg.pool_path_slot_rows(MP, T, H)
    bd, tk = Bound(vb, 2, R), TickOut(vb, pkg, kmax, 3 * frames)
    g0, g1 = Got(), Got()
    try:
        with _pool(vb, pkg, shape, 2, kmax, 0.0, T) as pool:
            bd.bind(pool)
            pool.push([(1, a_audio[:first]), (0, streams[0][0][:first])], **tk.kw())
            out = bd.take({0, 1})
            g0.add(out[0])
            old = out[1][3]
            assert old[0] == 0 and old[3] > 0 and old[1] + old[3] == 50            # frames are pending when the reset comes
            pool.reset_stream(1)
            pos0, pos1 = first, 0
            for i, sz in enumerate(rest):
                bd.clear()
                ents = [(1, b_audio[pos1:pos1 + sz])] + ([(0, streams[0][0][pos0:pos0 + s0[i + 1]])] if i + 1 < len(s0) else [])
                pool.push(ents, **tk.kw())
                out = bd.take({1, 0} if len(ents) == 2 else {1})
                g1.add(out[1])
                pos1 += sz
                if len(ents) == 2:
                    g0.add(out[0]); pos0 += s0[i + 1]
            assert g1.cm[0][0] == 0                                               # `first` restarts at 0: nothing of stream A is left
            assert pos0 == T and pos1 == T
            pool.mark_utterance(0); pool.mark_utterance(1)
            bd.clear()
            pool.push([], **tk.kw())
            out = bd.take({0, 1})
            g0.add(out[0]); g1.add(out[1])
            # mark, empty tick, reset: the old call's tail first, then a fresh slot
            pool.reset_stream(1)
            bd.clear()
            pool.push([(1, a_audio[:first])], **tk.kw())
            again = bd.take({1})[1]
            pool.mark_utterance(1)
            bd.clear()
            pool.push([], **tk.kw())
            tail = bd.take({1})[1]
            assert tail[3] == (old[1], old[3], 0, 0) and again[3] == old
            pool.reset_stream(1)
            bd.clear()
            pool.push([(1, b_audio[:rest[0]])], **tk.kw())
            fresh = bd.take({1})[1]
            assert fresh[3] == g1.cm[0] and np.array_equal(_u64(fresh[0]), _u64(g1.p[0]))
    finally:
        bd.free(); tk.free()
    want1 = _session(vb, pkg, ("t6", 1), b_audio, shape, kmax, 0.0, rest)
    _equal("the reset slot against a fresh bound session", g1, want1)
    want0 = _session(vb, pkg, ("t6", 0), streams[0][0], shape, kmax, 0.0, s0)
    _equal("the neighbour slot", g0, want0)
    # the old call's contour: its first tick and the tail the mark fetched are a session's push and mark on stream A
    wa = _session(vb, pkg, ("t6", "a"), a_audio, shape, kmax, 0.0, [first])
    ga = Got(); ga.add(again); ga.add(tail)
    _equal("mark, empty tick, then reset: the old call's tail", ga, wa)


# ---- 7. untouched memory -------------------------------------------------------------------------------------------------------------

def test_untouched_memory_and_an_unbound_pools_tick(vb, pkg, base):
    """path_ld 4: columns 2-3 of the rows, rows past n, the areas and records of unvisited slots keep their canaries (Bound.take
    checks all of it); and everything else a bound tick writes -- records, status rows, lists -- equals an unbound pool's tick"""
    shape, kmax, n = SMALL, 4, 4
    N, H = shape
    streams = gp._streams(base, "pcm16", shape, 5)[:n]
    blocks = [[N + 20 * H, 3 * H + 7, 1], [N + 5 * H, H, 7 * H], [N - 1, 1, 2 * H]]        # slot 3 is never listed
    R = pkg.pool_path_slot_rows(MP, N + 20 * H, H) + 5
    outs = []
    for bound in (True, False):
        bd, tk = Bound(vb, n, R, ld=4), TickOut(vb, pkg, kmax, 64)
        try:
            with _pool(vb, pkg, shape, n, kmax, 0.03, N + 20 * H) as pool:
                if bound:
                    bd.bind(pool)
                pos, per_tick = [0] * 3, []
                for t in range(3):
                    order = [2, 0, 1] if t % 2 else [0, 1, 2]
                    if t == 2:
                        order = [1, 2]                                           # slot 0 skips the tick: unvisited
                        pool.mark_utterance(1)
                    ents = [(k, streams[k][0][pos[k]:pos[k] + blocks[k][t]]) for k in order]
                    for k in order:
                        pos[k] += blocks[k][t]
                    tk.clear(); bd.clear()
                    rows, total = pool.push(ents, **tk.kw())
                    vb.sync()
                    per_tick.append([rows.copy(), total] + [d.numpy() for d in tk.all])
                    got = bd.take(set(order) if bound else set())
                    if bound and t == 0:
                        assert got[2][3] == (0, 0, 0, 0) and got[0][3][1] + got[0][3][3] == 21      # no frame yet: n = 0, nothing pending
                outs.append(per_tick)
        finally:
            bd.free(); tk.free()
    for a, b in zip(*outs):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        for x, y in zip(a[2:], b[2:]):
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


# ---- 8. launches ---------------------------------------------------------------------------------------------------------------------

def test_one_more_launch_whatever_the_number_of_entries(vb, pkg, base):
    shape, kmax, n = SMALL, 4, 40
    N, H = shape
    streams = gp._streams(base, "pcm16", shape, 130, 40)[:n]
    R = pkg.pool_path_slot_rows(MP, N, H)
    reports = {}
    for bound in (True, False):
        bd, tk = Bound(vb, n, R), TickOut(vb, pkg, kmax, 2 * n)
        try:
            with _pool(vb, pkg, shape, n, kmax, 0.03, N) as pool:
                if bound:
                    bd.bind(pool)
                pool.push([(k, streams[k][0][:N]) for k in range(n)], **tk.kw())
                pos = N
                for m in (1, 3, 40):                                             # steady state: one hop per entry
                    vb.sync()
                    vb.profile(True); vb.profile_reset()
                    pool.push([(k, streams[k][0][pos:pos + H]) for k in range(m)], **tk.kw())
                    vb.sync()
                    reports[(bound, m)] = {k: v[1] for k, v in vb.profile_report().items() if v[1]}
                    vb.profile(False)
                    pool.push([(k, streams[k][0][pos:pos + H]) for k in range(m, n)], **tk.kw())
                    pos += H
        finally:
            bd.free(); tk.free()
    for m in (1, 3, 40):
        want = dict(reports[(False, m)])
        assert "pitch_path_online_pool" not in want
        want["pitch_path_online_pool"] = 1
        assert reports[(True, m)] == want, (m, reports[(True, m)], want)
        assert "pitch_path_online" not in reports[(True, m)] and "pitch_path_online_all" not in reports[(True, m)]
    assert reports[(True, 1)] == reports[(True, 3)] == reports[(True, 40)]


# ---- 9. rejections -------------------------------------------------------------------------------------------------------------------

def test_rejections(vb, pkg, base):
    shape, kmax, n = SMALL, 4, 2
    N, H = shape
    frames = 40
    T = (frames - 1) * H + N
    streams = gp._streams(base, "pcm16", shape, 130, frames)[:n]
    L = vb.L
    mb = N + 9 * H
    R = pkg.pool_path_slot_rows(MP, mb, H)
    bd, tk = Bound(vb, n, R), TickOut(vb, pkg, kmax, 2 * frames)
    po = pkg.PoolPathOutputs(bd.path.ptr, bd.index.ptr, bd.forced.ptr, bd.commit.ptr)

    def refused(pool, peak_ref=1.0, mp=MP, out=po, ld=2, rows=R):
        rc = L.vbx_pool_path_bind(pool.handle if pool is not None else None, C.c_double(peak_ref), mp, None if out is None else C.byref(out), ld, rows)
        assert rc == E_INVALID, rc

    def ticks_fine(pool, slot, audio, bound):
        """the pool still ticks correctly: one block, the rows a bound session commits (or, unbound, nothing of the bound arrays)"""
        bd.clear()
        rows, total = pool.push([(slot, audio[:mb])], **tk.kw())
        assert total == pkg.frame_count(mb, N, H)
        got = bd.take({slot} if bound else set())
        if bound:
            g = Got(); g.add(got[slot])
            _equal("after a rejection", g, _session(vb, pkg, ("t9", slot), audio, shape, kmax, 0.03, [mb], final=False))

    try:
        refused(None)
        with vb.pool(sp._params(pkg), None, None, format=1, frame_len=N, stride=H, max_streams=n, max_block=mb) as plain:
            refused(plain)                                                       # no h_track
        with _pool(vb, pkg, shape, n, kmax, 0.03, mb) as pool:
            refused(pool, out=None)
            refused(pool, out=pkg.PoolPathOutputs(None, bd.index.ptr, bd.forced.ptr, bd.commit.ptr))
            refused(pool, out=pkg.PoolPathOutputs(bd.path.ptr, bd.index.ptr, bd.forced.ptr, None))
            refused(pool, ld=1)
            refused(pool, mp=0)
            refused(pool, mp=(1 << 24) + 1, rows=(1 << 24) + 1 + R)
            refused(pool, rows=R - 1)
            refused(pool, peak_ref=-1.0)
            refused(pool, peak_ref=float("inf"))
            refused(pool, peak_ref=float("nan"))
            ticks_fine(pool, 0, streams[0][0], False)                            # unbound and usable
            refused(pool)                                                        # a first bind after work was queued
            ticks_fine(pool, 1, streams[1][0], False)
        with _pool(vb, pkg, shape, n, kmax, 0.03, mb) as pool:
            bd.bind(pool)
            refused(pool, peak_ref=0.5)                                          # a rebind keeps peak_ref, max_pending and slot_rows
            refused(pool, mp=MP - 1)
            refused(pool, rows=R + 1)
            refused(pool, out=None)
            ticks_fine(pool, 0, streams[0][0], True)
            bd.bind(pool)                                                        # the same binding again: only the destinations, the state is kept
            bd.clear()
            pool.mark_utterance(0)
            pool.push([], **tk.kw())
            c = bd.take({0})[0][3]
            assert c[1] > 0 and c[3] == 0 and c[0] + c[1] == pkg.frame_count(mb, N, H)
    finally:
        bd.free(); tk.free()
