"""vbx_path_stream_*: the pitch path committed while the lists arrive (include/voxbox_hip.h).

What is held: the rows that are not flagged as forced are vbx_pitch_path_f64's, bit for bit, for every way of cutting the frames
into pushes; forced rows, flags and every push's commit record are the definition's (tests/pitch_path_online_model.py)."""
import ctypes as C

import numpy as np
import pytest

import layout_arena as la
import pitch_path_model as M
import pitch_path_online_model as O
import stream_harness as sh
from pitch_path_shard_model import early_stream, late_stream

pytestmark = pytest.mark.gpu

F = 600
i32, i64, u8, f64 = np.int32, np.int64, np.uint8, np.float64
SCHEDULES = ("whole", "one", "seven", "random")
_CACHE = {}


def _random_lists(rng, F, kmax, zero_frac=0.1):
    f = rng.uniform(60.0, 650.0, (F, kmax))
    f[rng.uniform(size=(F, kmax)) < zero_frac] = 0.0
    a = rng.uniform(0.0, 1.0, (F, kmax))
    cand = np.stack([f, a], axis=-1)
    count = rng.integers(0, kmax + 3, F).astype(i32)
    status = np.where(rng.uniform(size=F) < 0.03, rng.integers(1, 5, F), 0).astype(i32)
    lp = rng.uniform(0.0, 1.0, F) ** 3
    return cand, count, status, lp


def _sizes(schedule, n, seed=0):
    if schedule == "whole":
        return [n]
    if schedule in ("one", "seven"):
        k = 1 if schedule == "one" else 7
        return [k] * (n // k) + ([n % k] if n % k else [])
    rng = np.random.default_rng(77 + seed)
    out = []
    while sum(out) < n:
        out.append(int(min(n - sum(out), rng.choice([0, 0, 1, 2, 3, 5, 13, 40, 97]))))
    return out


def _case(kmax):
    """random lists of one kmax, uploaded once per module run: (host lists, device lists)"""
    if ("lists", kmax) not in _CACHE:
        _CACHE[("lists", kmax)] = _random_lists(np.random.default_rng(9000 + kmax), F, kmax)
    return _CACHE[("lists", kmax)]


def _model(key, tab_fn, mp, marks):
    if key not in _CACHE:
        tab = tab_fn()
        res = O.run(tab, mp, marks=marks)
        _CACHE[key] = (tab, res, M.outputs(tab, np.maximum(res["states"], 0)))
    return _CACHE[key]


class Lists:
    """the lists of a case in device memory, addressed by frame"""

    def __init__(self, vb, cand, count, status, lp):
        self.vb, self.kmax, self.F = vb, cand.shape[1], cand.shape[0]
        self.d = [vb.to_device(np.ascontiguousarray(cand, f64)), vb.to_device(count.astype(i32)),
                  None if status is None else vb.to_device(status.astype(i32)), None if lp is None else vb.to_device(lp.astype(f64))]

    def at(self, t):
        c, n, s, p = self.d
        return (c.ptr + t * self.kmax * 16, n.ptr + 4 * t, None if s is None else s.ptr + 4 * t, None if p is None else p.ptr + 8 * t)

    def free(self):
        for d in self.d:
            if d is not None:
                d.free()


def _drive(vb, ps, lists, sizes, ends=(), use_peak=True, t0=0):
    """Pushes of the given sizes, nothing waited for in between: every push has its own rows (max_pending + n of them) and its own
    commit record.  ends: the frame counts after which the push carries end_utterance.  Returns the concatenated committed rows
    (path, index, forced) and the commit records; asserts that rows beyond n were not touched."""
    mp = ps.max_pending
    rows = [mp + n for n in sizes]
    off = np.concatenate([[0], np.cumsum(rows)]).astype(int)
    tot = int(off[-1])
    path, idx, forced, com = vb.empty((tot, 2)), vb.empty(tot, i32), vb.empty(tot, u8), vb.empty((len(sizes), 4), i64)
    try:
        for d in (path, idx, forced, com):
            vb._check(vb.L.vbx_memset(vb.ctx, d.ptr, 0xFF, d.nbytes))
        t = t0
        for i, n in enumerate(sizes):
            c, k, s, p = lists.at(t)
            t += n
            ps.push(c, k, s, p if use_peak else None, n_frames=n, end_utterance=(t in ends),
                    out=(path.ptr + 16 * int(off[i]), idx.ptr + 4 * int(off[i]), forced.ptr + int(off[i]), com.ptr + 32 * i))
        vb.sync()
        ph, ih, fh, ch = path.numpy(), idx.numpy(), forced.numpy(), com.numpy()
    finally:
        for d in (path, idx, forced, com):
            d.free()
    gp, gi, gf = [], [], []
    for i in range(len(sizes)):
        n = int(ch[i, 1])
        assert 0 <= n <= rows[i], (i, ch[i])
        a, b = int(off[i]), int(off[i + 1])
        gp.append(ph[a:a + n]); gi.append(ih[a:a + n]); gf.append(fh[a:a + n])
        assert np.all(ph[a + n:b].view(np.uint64) == 0xFFFFFFFFFFFFFFFF) and np.all(ih[a + n:b] == -1) and np.all(fh[a + n:b] == 0xFF), i
    return np.concatenate(gp), np.concatenate(gi), np.concatenate(gf), [tuple(int(v) for v in r) for r in ch]


def _pushes(sizes, ends, t0=0):
    out, t = [], t0
    for n in sizes:
        t += n
        out.append((t, t in ends))
    return out


def _params(pkg, **kw):
    return pkg.PitchPathParams.make(**dict(dict(silence_threshold=0.0), **kw))


def _bits(a, b):
    return sh.bits_equal(np.ascontiguousarray(a), np.ascontiguousarray(b))


# ---- exact cases: every G from 4 to 64, four schedules -----------------------------------------------------------------------

@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("kmax", [2, 7, 15, 31, 63])
def test_committed_rows_are_the_resident_path(vb, pkg, kmax, schedule):
    cand, count, status, lp = _case(kmax)
    par = _params(pkg)
    if ("resident", kmax) not in _CACHE:
        _CACHE[("resident", kmax)] = vb.pitch_path(cand, count, status, None, params=par)
    want_p, want_i = _CACHE[("resident", kmax)]
    tab, res, _ = _model(("exact", kmax), lambda: M.frame_table(cand, count, status, None, None, dict(M.DEFAULTS, silence_threshold=0.0)), 64, [F])
    assert not res["forced"].any() and res["max_pending_seen"] < 64
    sizes = _sizes(schedule, F, kmax)
    lists = Lists(vb, cand, count, status, lp)
    try:
        with vb.path_stream(kmax, par, peak_ref=1.0, max_pending=64) as ps:
            gp, gi, gf, com = _drive(vb, ps, lists, sizes, ends={F}, use_peak=False)
    finally:
        lists.free()
    assert gp.shape == (F, 2) and _bits(gp, want_p)
    assert np.array_equal(gi, want_i)
    assert not gf.any()
    assert com == O.commits(res, _pushes(sizes, {F}))


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("kmax", [2, 7, 15, 31, 63])
def test_peak_ref_is_the_shard_protocols_seg_peak(vb, pkg, kmax, schedule):
    """silence_threshold > 0: P = peak_ref, which is what the world-1 shard calls compute with seg_peak = peak_ref"""
    cand, count, status, lp = _case(kmax)
    par = _params(pkg, silence_threshold=0.03)
    peak_ref = 0.8
    lists = Lists(vb, cand, count, status, lp)
    tmp = []
    try:
        if ("shard", kmax) not in _CACHE:
            pk = vb.to_device(np.array([peak_ref]))
            state, back, changed = vb.empty(64), vb.empty(64, i32), vb.empty(1, i32)
            path, index = vb.empty((F, 2)), vb.empty(F, i32)
            tmp += [pk, state, back, changed, path, index]
            c, k, s, p = lists.d
            vb.pitch_path_shard_begin(c, k, s, F, kmax, p, pk, None, par, 0, False, False)
            vb.pitch_path_shard_enter(None, state, back, changed)
            vb.pitch_path_shard_finish(None, path, 2, index)
            _CACHE[("shard", kmax)] = (path.numpy(), index.numpy())
        want_p, want_i = _CACHE[("shard", kmax)]
        tab, res, _ = _model(("peak", kmax), lambda: O.online_table(cand, count, status, lp, peak_ref, dict(M.DEFAULTS, silence_threshold=0.03)), 64, [F])
        assert not res["forced"].any()
        sizes = _sizes(schedule, F, kmax)
        with vb.path_stream(kmax, par, peak_ref=peak_ref, max_pending=64) as ps:
            gp, gi, gf, com = _drive(vb, ps, lists, sizes, ends={F})
    finally:
        lists.free()
        for d in tmp:
            d.free()
    assert np.any(want_p[:, 1][want_p[:, 0] == 0.0] > par.voicing_threshold)          # the silence term is at work
    assert _bits(gp, want_p) and np.array_equal(gi, want_i) and not gf.any()
    assert com == O.commits(res, _pushes(sizes, {F}))


# ---- forced cases ---------------------------------------------------------------------------------------------------------------

def _forced_case(name):
    if name == "late":
        cand, count = late_stream(F, 300)
        return cand, count, None, None, 16
    if name == "early":
        cand, count = early_stream(F, 300)
        return cand, count, None, None, 16
    cand, count, status, lp = _case(15)
    return cand, count, status, lp, 4


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", ["late", "early", "tiny_ring"])
def test_forced_rows_flags_and_commits_are_the_models(vb, pkg, name, schedule):
    cand, count, status, lp, mp = _forced_case(name)
    kmax = cand.shape[1]
    tab, res, (want_p, want_i) = _model(("forced", name), lambda: M.frame_table(cand, count, status, None, None, dict(M.DEFAULTS, silence_threshold=0.0)),
                                        mp, [F])
    assert res["forced"].any() and not res["forced"].all()
    sizes = _sizes(schedule, F, 3)
    lists = Lists(vb, cand, count, status, lp)
    try:
        with vb.path_stream(kmax, _params(pkg), max_pending=mp) as ps:
            gp, gi, gf, com = _drive(vb, ps, lists, sizes, ends={F}, use_peak=False)
    finally:
        lists.free()
    assert np.array_equal(gf.astype(bool), res["forced"])
    assert np.array_equal(gi, want_i) and _bits(gp, want_p)
    assert com == O.commits(res, _pushes(sizes, {F}))
    whole = M.outputs(tab, M.path_states(tab, None))
    ok = ~res["forced"]
    assert np.array_equal(gi[ok], whole[1][ok]) and _bits(gp[ok], whole[0][ok])      # what is not forced is the whole path


# ---- marks ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ("seven", "random"))
def test_marks_are_seg_start(vb, pkg, schedule):
    kmax = 7
    cand, count, status, lp = _case(kmax)
    par = _params(pkg)
    marks = [7, 14, 140, 301, F] if schedule == "seven" else None
    sizes = _sizes(schedule, F, 5)
    if marks is None:                                          # marks where the random schedule has push ends
        ends = np.cumsum(sizes)
        marks = sorted(set(int(ends[i]) for i in (1, 4, 9, len(sizes) // 2)) - {0}) + [F]
    seg = np.array([0] + [m for m in marks if m < F], i64)
    want_p, want_i = vb.pitch_path(cand, count, status, None, seg_start=seg, params=par)
    tab = M.frame_table(cand, count, status, None, None, dict(M.DEFAULTS, silence_threshold=0.0))
    res = O.run(tab, 64, marks=marks)
    lists = Lists(vb, cand, count, status, lp)
    try:
        with vb.path_stream(kmax, par, max_pending=64) as ps:
            gp, gi, gf, com = _drive(vb, ps, lists, sizes, ends=set(marks), use_peak=False)
    finally:
        lists.free()
    assert _bits(gp, want_p) and np.array_equal(gi, want_i) and not gf.any()
    assert com == O.commits(res, _pushes(sizes, set(marks)))
    for c, (T, end) in zip(com, _pushes(sizes, set(marks))):
        if end:
            assert c[3] == 0 and c[0] + c[1] == T              # a mark delivers the rest at once


def test_a_zero_frame_push_can_carry_the_mark_and_reset_starts_over(vb, pkg):
    kmax = 7
    cand, count, status, lp = _case(kmax)
    par = _params(pkg)
    n = 100
    want_p, want_i = vb.pitch_path(cand[:n], count[:n], status[:n], None, params=par)
    with vb.path_stream(kmax, par, max_pending=64) as ps:
        p0, i0, f0, c0 = ps.push(cand[:n], count[:n], status[:n])
        assert c0[0] == 0 and c0[1] + c0[3] == n
        p1, i1, f1, c1 = ps.push(cand[:0], count[:0], status[:0], end_utterance=True)
        assert c1 == (c0[1], c0[3], 0, 0)
        assert _bits(np.concatenate([p0, p1]), want_p) and np.array_equal(np.concatenate([i0, i1]), want_i)
        p2, _, _, c2 = ps.push(cand[:0], count[:0], status[:0], end_utterance=True)       # nothing pending: nothing written
        assert c2 == (n, 0, 0, 0) and p2.shape == (0, 2)
        ps.push(cand[:40], count[:40], status[:40])                                        # ... leave frames pending, then reset
        ps.reset()
        p3, i3, _, c3 = ps.push(cand[:n], count[:n], status[:n], end_utterance=True)
        assert c3 == (0, n, 0, 0) and _bits(p3, want_p) and np.array_equal(i3, want_i)


# ---- layout: path_ld 7 inside a fenced arena ----------------------------------------------------------------------------------

def test_path_ld_7_in_a_fenced_arena(vb, pkg):
    kmax, n, mp, ld = 15, 150, 8, 7
    cand, count, status, lp = _case(kmax)
    cand, count, status = cand[:n], count[:n], status[:n]
    tab = M.frame_table(cand, count, status, None, None, dict(M.DEFAULTS, silence_threshold=0.0))
    res = O.run(tab, mp, marks=[n])
    want_p, want_i = M.outputs(tab, res["states"])
    rows = mp + n
    a = la.Arena(la.DeviceBackend(vb), "path_stream/ld7")
    a.input("cand", cand, residue=8)
    a.input("count", count, residue=4)
    a.input("status", status, residue=12)
    a.output("path", f64, rows, 2, ld=ld, residue=8)
    a.output("index", i32, rows, 1, residue=4)
    a.output("forced", i32, (rows + 3) // 4, 1, residue=12)     # (bytes; the arena's canaries are words)
    a.output("commit", i32, 8, 1, residue=8)
    a.place()
    with vb.path_stream(kmax, _params(pkg), max_pending=mp) as ps:
        ps.push(a["cand"], a["count"], a["status"], None, n_frames=n, end_utterance=True,
                out=(a["path"], a["index"], a["forced"], a["commit"]), path_ld=ld)
        vb.sync()
    out = a.finish()
    com = tuple(int(v) for v in out["commit"].reshape(-1).view(i64))
    assert com == (0, n, int(res["forced"].sum()), 0) and com[2] > 0
    assert _bits(out["path"][:n], want_p) and np.array_equal(out["index"][:n, 0], want_i)
    fb = out["forced"].reshape(-1).view(u8)
    assert np.array_equal(fb[:n].astype(bool), res["forced"])
    # rows beyond n still hold the canaries
    assert la.unwritten(out["path"][n:]).shape[0] == (rows - n) * 2 and la.unwritten(out["index"][n:]).shape[0] == rows - n
    assert np.array_equal(fb[n:], np.full(fb.size // 4, la.CANARY_I32, np.uint32).view(u8)[n:])


# ---- two streams on one context, interleaved -------------------------------------------------------------------------------------

def test_two_streams_on_one_context_interleaved(vb, pkg):
    par = _params(pkg)
    ca, cb = _case(7), _case(31)
    la_, lb = Lists(vb, *ca), Lists(vb, *cb)
    want = [vb.pitch_path(c[0], c[1], c[2], None, params=par) for c in (ca, cb)]
    try:
        with vb.path_stream(7, par, max_pending=64) as pa, vb.path_stream(31, par, max_pending=64) as pb:
            got = [[], []]
            t = [0, 0]
            rng = np.random.default_rng(12)
            while min(t) < F:
                w = int(rng.integers(0, 2))
                if t[w] >= F:
                    w ^= 1
                n = int(min(F - t[w], rng.integers(1, 30)))
                ps, ls = (pa, la_) if w == 0 else (pb, lb)
                gp, gi, gf, _ = _drive(vb, ps, ls, [n], ends={F}, use_peak=False, t0=t[w])
                t[w] += n
                got[w].append((gp, gi))
                assert not gf.any()
    finally:
        la_.free(); lb.free()
    for w in (0, 1):
        assert _bits(np.concatenate([g[0] for g in got[w]]), want[w][0]) and np.array_equal(np.concatenate([g[1] for g in got[w]]), want[w][1])


# ---- stream order ------------------------------------------------------------------------------------------------------------------

def test_push_behind_a_late_producer(pkg, vb):
    """The lists arrive late on the stream and are overwritten right behind the push: the rows come from the stream's own ring"""
    hip = sh.Hip(pkg)
    stream = hip.stream_create()
    v = pkg.VoxBox(0, stream)
    try:
        delay = sh.Delay(v, pkg)
        kmax, mp = 15, 64
        cand_h, count_h, status_h, lp_h = _case(kmax)
        par = _params(pkg, silence_threshold=0.03)
        cand, cnt, st, peak = v.empty((F, kmax, 2)), v.empty(F, i32), v.empty(F, i32), v.empty(F)
        rows = mp + 400
        outs = (v.empty((rows, 2)), v.empty(rows, i32), v.empty(rows, u8), v.empty(4, i64))
        ps = v.path_stream(kmax, par, peak_ref=0.8, max_pending=mp)
        cand_true = v.to_device(cand_h)

        def call():
            # a first push whose lists are gone when the second commits their pending frames: the second push's lists are then
            # poisoned behind it as well
            ps.reset()
            ps.push(cand, cnt, st, peak, n_frames=200, out=outs)
            hip.memset_async(cand.ptr, 0xFF, 200 * kmax * 16, stream)
            ps.push(cand.ptr + 200 * kmax * 16, cnt.ptr + 800, st.ptr + 800, peak.ptr + 1600, n_frames=400, end_utterance=True, out=outs)
            hip.copy_async(cand.ptr, cand_true.ptr, 200 * kmax * 16, stream)                    # (restored for the input check)
        r = sh.late_producer(v, stream, call, [(cand, cand_h), (cnt, count_h), (st, status_h), (peak, lp_h)], list(outs), delay, hip=hip)
        assert r["streams"].get("pitch_path_online") == 0
        tab = O.online_table(cand_h, count_h, status_h, lp_h, 0.8, dict(M.DEFAULTS, silence_threshold=0.03))
        res = O.run(tab, mp, marks=[F])
        c200 = int(res["before_mark"][200])
        want_p, want_i = M.outputs(tab, res["states"])
        com = tuple(int(x) for x in r["ref"][3])
        assert com == (c200, F - c200, 0, 0) and 200 - c200 >= 1
        assert _bits(r["ref"][0][:F - c200], want_p[c200:]) and np.array_equal(r["ref"][1][:F - c200], want_i[c200:])
        ps.close()
    finally:
        v.sync()
        v.close()
        hip.stream_sync(stream)
        hip.stream_destroy(stream)


# ---- rejections and the profile ---------------------------------------------------------------------------------------------------

def test_every_rejection_leaves_context_and_stream_usable(vb, pkg):
    L = vb.L
    h = C.c_void_p()
    good = _params(pkg)

    def opens(kmax, par, peak, mp, ctx=vb.ctx):
        rc = L.vbx_path_stream_open(ctx, kmax, None if par is None else C.byref(par), peak, mp, C.byref(h))
        assert not h.value or rc == 0
        return rc
    assert opens(0, good, 1.0, 8) == -1 and opens(64, good, 1.0, 8) == -1                      # kmax 0 or above 63
    assert opens(4, good, 1.0, 0) == -1                                                        # max_pending 0
    assert opens(4, None, 1.0, 8) == -1 and opens(4, good, 1.0, 8, ctx=None) == -1
    assert L.vbx_path_stream_open(vb.ctx, 4, C.byref(good), 1.0, 8, None) == -1
    for bad in (dict(time_step=0.0), dict(ceiling_hz=0.0), dict(octave_cost=-1.0), dict(voicing_threshold=float("nan"))):   # check_pitch_path's
        assert opens(4, _params(pkg, **bad), 1.0, 8) == -1, bad
    sil = _params(pkg, silence_threshold=0.03)
    for peak in (-1.0, float("nan"), float("inf")):                                            # silence needs a usable peak_ref
        assert opens(4, sil, peak, 8) == -1, peak
    assert opens(4, good, float("nan"), 8) == 0                                                # ... which silence 0 ignores
    L.vbx_path_stream_close(h)
    cand, count, status, lp = _case(7)
    lists = Lists(vb, cand, count, status, lp)
    path, idx, fo, com = vb.empty((80, 2)), vb.empty(80, i32), vb.empty(80, u8), vb.empty(4, i64)
    try:
        with vb.path_stream(7, sil, peak_ref=0.8, max_pending=16) as ps:
            c, k, s, p = lists.at(0)
            push = lambda *a: L.vbx_path_stream_push(*a)
            assert push(None, c, k, s, p, 8, 0, path.ptr, 2, idx.ptr, fo.ptr, com.ptr) == -1                 # NULL stream
            assert push(ps.handle, c, k, s, p, 8, 0, None, 2, idx.ptr, fo.ptr, com.ptr) == -1                # NULL outputs
            assert push(ps.handle, c, k, s, p, 8, 0, path.ptr, 2, idx.ptr, fo.ptr, None) == -1
            assert push(ps.handle, c, k, s, p, 8, 0, path.ptr, 1, idx.ptr, fo.ptr, com.ptr) == -1            # path_ld < 2
            assert push(ps.handle, None, k, s, p, 8, 0, path.ptr, 2, idx.ptr, fo.ptr, com.ptr) == -1         # NULL lists with frames
            assert push(ps.handle, c, None, s, p, 8, 0, path.ptr, 2, idx.ptr, fo.ptr, com.ptr) == -1
            assert push(ps.handle, c, k, s, None, 8, 0, path.ptr, 2, idx.ptr, fo.ptr, com.ptr) == -1         # silence > 0, no local_peak
            assert L.vbx_path_stream_reset(None) == -1 and L.vbx_path_stream_close(None) is None
            # nothing was queued by any of them: the stream still gives the whole path
            gp, gi, gf, cm = ps.push(cand[:60], count[:60], status[:60], lp[:60], end_utterance=True)
            tab = O.online_table(cand[:60], count[:60], status[:60], lp[:60], 0.8, dict(M.DEFAULTS, silence_threshold=0.03))
            want_p, want_i = M.outputs(tab, M.path_states(tab, None))
            assert cm[1] == 60 and cm[3] == 0 and np.array_equal(gi[~gf.astype(bool)], want_i[~gf.astype(bool)])
            assert _bits(gp[~gf.astype(bool)], want_p[~gf.astype(bool)])
    finally:
        lists.free()
        for d in (path, idx, fo, com):
            d.free()


def test_the_kernel_is_profiled_as_pitch_path_online(vb, pkg):
    cand, count, status, lp = _case(7)
    vb.profile(True)
    vb.profile_reset()
    try:
        with vb.path_stream(7, _params(pkg)) as ps:
            ps.push(cand[:50], count[:50], status[:50])
            ps.push(cand[50:60], count[50:60], status[50:60], end_utterance=True)
        rep = vb.profile_report()
    finally:
        vb.profile(False)
    assert rep["pitch_path_online"][1] == 2 and rep["pitch_path_online"][0] > 0.0
    assert vb.profile_streams()["pitch_path_online"] == 0
