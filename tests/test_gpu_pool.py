"""A session pool (vbx_pool_*) on a real MI355X: many independent live streams fed by ticks of (slot, block) entries, against the
yardsticks that are never the new code -- the one-channel vbx_session pushed the same blocks, marks and resets (push by push, canaries
included), the RESIDENT call on every stream's whole recording, and vbx_analyze_clips where a whole-stream comparison over hundreds of
streams must be fast.  Nothing is compared with a tolerance: records, the three status rows and, tracked, lists, counts and peaks are
compared on uint64 / integer views into canary-filled arrays, and NO case is left out of any comparison (share of cases skipped: 0).
Shapes: 400/160 (frames the kernels widen) and 1200/480 (the direct PCM16 / F32 readers), F = 200 frames per stream -- past the point
where the warm-up saturates at 64 frames.  Every stream has its own content (test_gpu_session_channels._mix), so a slot mix-up cannot
pass.  References are computed once per key."""
import ctypes as C

import numpy as np
import pytest

import layout_arena as la
import sample8_cases as s8
import test_gpu_analyze_host as ah
import test_gpu_session as gs
from test_gpu_session import base  # noqa: F401  (the module's recording fixture)
from test_gpu_session_channels import _mix, _same

pytestmark = pytest.mark.gpu

F = gs.F
KMAX = gs.KMAX
NATIVE, SMALL = (1200, 480), (400, 160)
E_INVALID = -1
CODE = {"pcm16": 1, "pcm24": 2, "pcm32": 3, "f32": 4, "f64": 5, "u8": 16, "ulaw": 17, "alaw": 18}
FORMATS = list(CODE)
FORMS = ["plain", "tracked", "tracked_ext"]
_u64 = gs._u64
_REC, _SESS, _RES = {}, {}, {}


def _streams(base, fmt, shape, n, frames=F):
    """n streams of `frames` frames, every one its own content: [(host audio as pushed, typed samples for the resident call, which call)]"""
    key = (fmt, shape, n, frames)
    if key not in _REC:
        N, H = shape
        y = _mix(base, n, (frames - 1) * H + N)
        out = []
        for k in range(n):
            x = np.ascontiguousarray(y[:, k])
            if fmt == "pcm16":
                a = np.round(x * 32767.0).astype(np.int16)
                out.append((a, a, "pcm16"))
            elif fmt == "pcm24":
                v = np.round(x * 8388607.0).astype(np.int32)
                out.append((ah._pack24(v), v.astype(np.float64) / np.float64(8388607.0), "f64"))
            elif fmt == "pcm32":
                a = np.round(x * 2147483647.0).astype(np.int64).astype(np.int32)
                out.append((a, a.astype(np.float64) / np.float64(2147483647.0), "f64"))
            elif fmt == "f32":
                a = x.astype(np.float32)
                out.append((a, a, "f32in"))
            elif fmt == "f64":
                out.append((x, x, "f64"))
            else:
                codes = s8.encode(CODE[fmt], np.round(x * 32767.0).astype(np.int16))
                out.append((codes, s8.decode(CODE[fmt], codes), "f64" if fmt == "u8" else "pcm16"))
        _REC[key] = out
    return _REC[key]


def _blk(audio, fmt, a, b):
    return audio[3 * a:3 * b] if fmt == "pcm24" else audio[a:b]


def _sizes(rng, N, H, T, big_first):
    """a ragged schedule that sums to T: a 1-sample block first (a tick that completes no frame), then -- for some streams -- more than
    64 frames at once, then draws from the menu"""
    menu = [1, H - 1, H, 3 * H + 7, 3 * H + 7, 7 * H + 3, 11 * H]
    sizes = [1] + ([N + 79 * H] if big_first else [N + 30 * H, 1, H - 1])
    while sum(sizes) < T:
        sizes.append(int(menu[int(rng.integers(0, len(menu)))]))
    sizes[-1] -= sum(sizes) - T
    if sizes[-1] == 0:
        sizes.pop()
    assert sum(sizes) == T and min(sizes) >= 1
    return sizes


def _ticks(rng, scheds):
    """which streams push their next block in which tick: tick 0 holds every stream (1 sample each: no frame), streams skip ticks at
    random, every fifth tick holds one entry, the entry order is shuffled"""
    nxt = [0] * len(scheds)
    ticks = [list(range(len(scheds)))]
    for k in ticks[0]:
        nxt[k] = 1
    while any(nxt[k] < len(scheds[k]) for k in range(len(scheds))):
        live = [k for k in range(len(scheds)) if nxt[k] < len(scheds[k])]
        if len(ticks) % 5 == 4:
            pick = [live[int(rng.integers(0, len(live)))]]
        else:
            pick = [k for k in live if rng.random() < 0.6] or [live[0]]
        pick = [pick[i] for i in rng.permutation(len(pick))]
        for k in pick:
            nxt[k] += 1
        ticks.append(pick)
    return ticks


class Acc:
    """what gs.Outputs.download() returns for one stream, kept on the host: canary-filled, a tick's rows copied to their frames"""

    def __init__(self, o):
        self.arrs = [np.full((o.F, o.ld), np.nan), np.full((3, o.F), -1, np.int32)]
        self.arrs[0].view(np.uint64)[...] = 0xFFFFFFFFFFFFFFFF
        if o.tracked:
            self.arrs += [np.empty((o.F, KMAX, 2)), np.full(o.F, -1, np.int32), np.empty(o.F)]
            self.arrs[2].view(np.uint64)[...] = 0xFFFFFFFFFFFFFFFF
            self.arrs[4].view(np.uint64)[...] = 0xFFFFFFFFFFFFFFFF

    def put(self, lo, got, r0, n):
        self.arrs[0][lo:lo + n] = got[0][r0:r0 + n]
        self.arrs[1][:, lo:lo + n] = got[1][:, r0:r0 + n]
        for k in range(2, len(self.arrs)):
            self.arrs[k][lo:lo + n] = got[k][r0:r0 + n]

    def upload(self, vb, o):
        for d, a in zip([o.rec, o.st] + o.lists, self.arrs):
            vb._check(vb.L.vbx_memcpy_h2d(vb.ctx, d.ptr, np.ascontiguousarray(a).ctypes.data, a.nbytes))


class Tick:
    """one tick's device outputs: rows [0, cap) and a fence of `extra` rows behind them, all canaries before the push"""

    def __init__(self, vb, o, cap, extra=3):
        self.vb, self.o, self.cap, self.n = vb, o, cap, cap + extra
        n = self.n
        self.rec, self.st = vb.empty((n, o.ld)), vb.empty((3, n), np.int32)
        self.lists = [vb.empty((n, KMAX, 2)), vb.empty(n, np.int32), vb.empty(n)] if o.tracked else []

    def clear(self):
        for d in [self.rec, self.st] + self.lists:
            self.vb._check(self.vb.L.vbx_memset(self.vb.ctx, d.ptr, 0xFF, d.nbytes))

    def kw(self):
        outs = tuple(d.ptr for d in self.lists) + (None,) if self.lists else None
        return dict(out=self.rec.ptr, status=self.st.ptr, outputs=outs, record_ld=self.o.ld, status_ld=self.n)

    def download(self, total):
        """the tick's arrays; everything outside rows [0, total) must still be the canary"""
        got = [self.rec.numpy(), self.st.numpy()] + [d.numpy() for d in self.lists]
        assert np.all(got[0][total:].view(np.uint64) == 0xFFFFFFFFFFFFFFFF) and np.all(got[1][:, total:] == -1), "rows past total_rows were written"
        assert np.all(got[0][:total, self.o.width:].view(np.uint64) == 0xFFFFFFFFFFFFFFFF), "the records' padding column was written"
        for a in got[2:]:
            assert np.all(np.ascontiguousarray(a[total:]).view(np.uint8) == 0xFF), "list rows past total_rows were written"
        return got

    def free(self):
        for d in [self.rec, self.st] + self.lists:
            d.free()


def _open_pool(vb, pkg, fmt, shape, form, n, max_block, max_tick=None):
    ext, track = ah._form(pkg, form)
    return vb.pool(ah._params(pkg), ext, track, format=CODE[fmt], frame_len=shape[0], stride=shape[1], max_streams=n, max_block=max_block,
                   max_tick=max_tick)


def _open_sess(vb, pkg, fmt, shape, form, max_block):
    ext, track = ah._form(pkg, form)
    return vb.session(ah._params(pkg), ext, track, format=CODE[fmt], channels=1, channel=0, frame_len=shape[0], stride=shape[1], max_block=max_block)


def _run_pool(vb, pkg, pool, o0, streams, fmt, scheds, ticks, marks=None, frames=F, pusher=None, between=None, extra_entries=False):
    """feeds the ticks; returns one Acc per stream.  marks: {stream: frames at which an utterance is marked}"""
    n = len(streams)
    accs = [Acc(o0) for _ in range(n)]
    pos, nxt = [0] * n, [0] * n
    cap = max(sum(max(s) for s in scheds) // pool.stride + n + 2, 4)
    tk = Tick(vb, o0, cap)
    for ti, pick in enumerate(ticks):
        entries = []
        for k in pick:
            lo = pool.info(k)[1]
            if marks and lo in marks.get(k, ()):
                pool.mark_utterance(k)
            sz = scheds[k][nxt[k]]
            entries.append((k, _blk(streams[k][0], fmt, pos[k], pos[k] + sz), sz))
        los = [pool.info(k)[1] for k, _, _ in entries]
        tk.clear()
        push_entries = [(k, b) for k, b, _ in entries]
        if extra_entries and ti % 3 == 1:                                         # an entry without samples: a no-op with zero rows
            idle = [k for k in range(n) if k not in pick]
            if idle:
                push_entries.insert(len(push_entries) // 2, (idle[0], _blk(streams[idle[0]][0], fmt, 0, 0)))
                entries.insert(len(entries) // 2, (idle[0], _blk(streams[idle[0]][0], fmt, 0, 0), 0))
                los.insert(len(los) // 2, pool.info(idle[0])[1])
        want_rows, want_total = pool.rows_of([(k, sz) for k, _, sz in entries])
        if pusher is None:
            rows, total = pool.push(push_entries, **tk.kw())
        else:
            rows, total = pusher(pool, entries, tk.kw())
        assert total == want_total and np.array_equal(rows, want_rows), (ti, rows, want_rows)
        got = tk.download(total)
        for (k, _, sz), lo, (r0, nr) in zip(entries, los, rows):
            accs[k].put(lo, got, int(r0), int(nr))
            if sz:
                pos[k] += sz
                nxt[k] += 1
            assert pool.info(k)[:2] == (pos[k], lo + int(nr))
        if between is not None:
            between(ti)
    tk.free()
    assert all(pool.info(k)[1] == frames for k in range(n)), [pool.info(k) for k in range(n)]
    return accs


def _session_outputs(vb, pkg, key, stream, fmt, shape, form, sizes, marks=()):
    """the one-channel session pushed the same blocks and marks: its Outputs download, computed once per key"""
    if key not in _SESS:
        o = gs.Outputs(vb, pkg, form)
        with _open_sess(vb, pkg, fmt, shape, form, max(sizes)) as sess:
            pos = 0
            for sz in sizes:
                lo = sess.info()[1]
                if lo in marks:
                    sess.mark_utterance()
                assert sess.push(_blk(stream[0], fmt, pos, pos + sz), **o.at(lo)) is None
                pos += sz
            assert sess.info()[1] == F
        _SESS[key] = o.download()
        o.free()
    return _SESS[key]


def _resident(vb, pkg, key, stream, shape, form, seg=None):
    return gs._reference(vb, pkg, stream[1], stream[2], shape, form, seg, key=("pool",) + key)


def _check(vb, pkg, base, fmt, shape, form, n=5, seed=1, marks=None, resident=True, pusher=None, between=None, key=(), policy="EXACT"):
    N, H = shape
    T = (F - 1) * H + N
    streams = _streams(base, fmt, shape, n)
    rng = np.random.default_rng(4000 + seed)
    scheds = [_sizes(rng, N, H, T, big_first=k % 2 == 0) for k in range(n)]
    ticks = _ticks(rng, scheds)
    assert any(len(t) == 1 for t in ticks) and any(len(t) < n for t in ticks) and len(ticks[0]) == n
    o0 = gs.Outputs(vb, pkg, form)
    with _open_pool(vb, pkg, fmt, shape, form, n, max(max(s) for s in scheds)) as pool:
        assert pool.push([], out=None)[0].shape == (0, 2)                        # an empty tick
        accs = _run_pool(vb, pkg, pool, o0, streams, fmt, scheds, ticks, marks, pusher=pusher, between=between, extra_entries=True)
    for k in range(n):
        mk = tuple(sorted(marks.get(k, ()))) if marks else ()
        label = f"{fmt} {shape} {form} stream {k} of {n}"
        want = _session_outputs(vb, pkg, (fmt, shape, form, n, k, seed, mk, policy) + key, streams[k], fmt, shape, form, scheds[k], mk)
        _same(label + ": the one-channel session", tuple(accs[k].arrs), want)
        if resident:
            seg = [0] + [m for m in mk if m > 0] if mk else None
            accs[k].upload(vb, o0)
            gs._assert_session(label + ": the resident call", vb, pkg, o0, _resident(vb, pkg, (fmt, shape, form, n, k, tuple(seg or ()), policy), streams[k],
                                                                                      shape, form, seg), shape, form, seg)
    o0.free()


# ---- 1. every format and form, ragged schedules, ragged ticks --------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_and_form(vb, pkg, base, fmt, form):
    _check(vb, pkg, base, fmt, SMALL, form)


@pytest.mark.parametrize("fmt", ["pcm16", "f32", "ulaw"])
def test_the_native_shape(vb, pkg, base, fmt):
    _check(vb, pkg, base, fmt, NATIVE, "tracked_ext", seed=2)


# ---- 2. utterance marks -----------------------------------------------------------------------------------------------------------

def test_marks_at_different_frames_per_stream(vb, pkg, base):
    """marks wherever a stream's delivered frames reach them (the schedules make different streams reach different frames); stream 3
    is marked before its first frame (frame 0: no entry of its own in h_seg_start) and stream 1 twice in a row (the same frame)"""
    N, H = SMALL
    T = (F - 1) * H + N
    rng = np.random.default_rng(4100)
    scheds = [_sizes(rng, N, H, T, big_first=k % 2 == 0) for k in range(5)]
    reach = []                                                                   # the frames each stream has delivered when a push begins
    for s in scheds:
        c, fr = 0, []
        for sz in s:
            fr.append(pkg.frame_count(c, N, H))
            c += sz
        reach.append(sorted(set(fr)))
    marks = {0: {reach[0][len(reach[0]) // 3], reach[0][2 * len(reach[0]) // 3]}, 1: {reach[1][len(reach[1]) // 2]},
             2: {r for r in reach[2] if 60 < r < 140 and r % 3 == 0}, 3: {0, reach[3][-3]}}
    assert all(marks.values()) and len({tuple(sorted(m)) for m in marks.values()}) == 4
    _check(vb, pkg, base, "pcm16", SMALL, "tracked_ext", seed=100, marks=marks)


# ---- 3. a slot is reset and reused ------------------------------------------------------------------------------------------------

def test_reset_stream_reuses_a_slot(vb, pkg, base):
    """slot 1 is fed 90 frames of stream A, reset, and then fed stream B's whole recording: its rows equal a fresh session's on B; the
    other slots go on undisturbed"""
    form, fmt, shape = "tracked_ext", "ulaw", SMALL
    N, H = shape
    T = (F - 1) * H + N
    streams = _streams(base, fmt, shape, 4)
    rng = np.random.default_rng(4200)
    scheds = [_sizes(rng, N, H, T, big_first=k % 2 == 0) for k in range(3)]
    o0 = gs.Outputs(vb, pkg, form)
    other = streams[3]
    first = N + 89 * H
    with _open_pool(vb, pkg, fmt, shape, form, 3, max(first, max(max(s) for s in scheds))) as pool:
        tk = Tick(vb, o0, 200)
        tk.clear()
        rows, total = pool.push([(1, _blk(other[0], fmt, 0, first))], **tk.kw())
        assert total == 90 and pool.info(1) == (first, 90, pool.info(1)[2])
        part = tk.download(total)
        want = gs._reference(vb, pkg, other[1], other[2], shape, form, None, key=("pool-reset", fmt, shape, form))
        assert np.array_equal(_u64(part[0][:90, 2:o0.width]), _u64(want[0][:90, 2:o0.width])) and np.array_equal(part[1][:, :90], want[1][:, :90])
        tk.free()
        pool.reset_stream(1)
        assert pool.info(1) == (0, 0, 0)
        ticks = _ticks(rng, scheds)
        accs = _run_pool(vb, pkg, pool, o0, streams[:3], fmt, scheds, ticks)
    for k in range(3):
        want = _session_outputs(vb, pkg, ("reset", fmt, shape, form, k), streams[k], fmt, shape, form, scheds[k])
        _same(f"slot {k} after slot 1 was reset", tuple(accs[k].arrs), want)
    o0.free()


# ---- 4. isolation -----------------------------------------------------------------------------------------------------------------

def test_a_nan_in_one_stream_touches_no_other(vb, pkg, base):
    """NaN and Inf samples in stream 2 -- across a block cut and at the very end of a plane region, right before the zero gap: the
    other streams' arrays equal a clean run's, bit for bit"""
    form, fmt, shape = "tracked_ext", "f32", SMALL
    N, H = shape
    T = (F - 1) * H + N
    clean = _streams(base, fmt, shape, 4)
    sizes = [N + 69 * H] + [H] * 40 + [7, H - 7] + [3 * H] * 29 + [2 * H]
    assert sum(sizes) == T
    scheds = [sizes] * 4
    ticks = [[0, 1, 2, 3]] * len(sizes)
    bad = clean[2][0].copy()
    cut = sizes[0]
    bad[cut - 2:cut + 3] = np.array([np.nan, np.inf, -np.inf, np.nan, np.inf], np.float32)      # across the first block cut
    end = sum(sizes[:5])
    bad[end - 1] = np.nan                                                                          # the last sample of a region
    bad[end + 40 * H - 3:end + 40 * H] = np.inf
    runs = []
    for audio2 in (clean[2][0], bad):
        streams = [clean[0], clean[1], (audio2, None, None), clean[3]]
        o0 = gs.Outputs(vb, pkg, form)
        with _open_pool(vb, pkg, fmt, shape, form, 4, max(sizes)) as pool:
            runs.append(_run_pool(vb, pkg, pool, o0, streams, fmt, scheds, ticks))
        o0.free()
    for k in (0, 1, 3):
        _same(f"stream {k} beside a stream with NaN / Inf", tuple(runs[1][k].arrs), tuple(runs[0][k].arrs))
    assert not np.array_equal(_u64(runs[1][2].arrs[0]), _u64(runs[0][2].arrs[0]))                  # (the bad stream itself differs)
    want = _session_outputs(vb, pkg, ("isolation", 0), clean[0], fmt, shape, form, sizes)
    _same("stream 0 against its session", tuple(runs[1][0].arrs), want)


# ---- 5. 300 streams against vbx_analyze_clips ----------------------------------------------------------------------------------------

def test_three_hundred_streams_equal_analyze_clips(vb, pkg, base):
    """300 mu-law streams at 200/80 (past 64 and past 256 entries a tick): recordings of 12 to 90 frames of differing lengths, fed
    in two-hop packets with staggered starts and ends; every stream's concatenated rows equal vbx_analyze_clips' rows for that whole
    recording -- one existing call, by its contract the resident rows"""
    N, H, n, form = 200, 80, 300, "tracked"
    rng = np.random.default_rng(4500)
    ext, track = ah._form(pkg, form)
    pcm = np.round(base * 0.9 * 32767.0).astype(np.int16)
    frames = [12 + int(v) for v in rng.integers(0, 79, n)]
    frames[:2] = [12, 90]
    lens = [(f - 1) * H + N + int(rng.integers(0, H)) for f in frames]
    starts = [int(v) for v in rng.integers(0, 5, n)]                              # the tick a stream's first packet arrives in
    recs = []
    for k in range(n):
        a = int(rng.integers(0, pcm.size - lens[k]))
        sig = (pcm[a:a + lens[k]].astype(np.int32) * (40 + k % 60) // 100).astype(np.int16)      # its own window, its own level
        recs.append(s8.encode(s8.ULAW, sig))
    dev = [vb.to_device(r, np.uint8) for r in recs]
    want = vb.analyze_clips(dev, lens, ah._params(pkg), ext, track, format=s8.ULAW, frame_len=N, stride=H, lists=True)
    for d in dev:
        d.free()
    starts_row = np.concatenate([[0], np.cumsum(frames)])
    width = ah._width(vb, pkg, form)
    ld = width + (width & 1)
    got_rec = np.zeros((starts_row[-1], ld))
    got_st = np.zeros((3, starts_row[-1]), np.int32)
    got_cand, got_count, got_peak = np.zeros((starts_row[-1], KMAX, 2)), np.zeros(starts_row[-1], np.int32), np.zeros(starts_row[-1])
    o0 = gs.Outputs(vb, pkg, form, 4)
    P = 2 * H
    most = 0
    with vb.pool(ah._params(pkg), ext, track, format=s8.ULAW, frame_len=N, stride=H, max_streams=n, max_block=P, max_tick=n * P) as pool:
        tk = Tick(vb, o0, 3 * n)
        pos, t = [0] * n, 0
        while any(pos[k] < lens[k] for k in range(n)):
            live = [k for k in range(n) if starts[k] <= t and pos[k] < lens[k]]
            live = [live[i] for i in rng.permutation(len(live))]
            if live:
                most = max(most, len(live))
                tk.clear()
                rows, total = pool.push([(k, recs[k][pos[k]:pos[k] + P]) for k in live], **tk.kw())
                got = tk.download(total)
                for k, (r0, nr) in zip(live, rows):
                    lo = pool.info(k)[1] - int(nr)
                    a, r0, nr = int(starts_row[k]) + lo, int(r0), int(nr)
                    got_rec[a:a + nr], got_st[:, a:a + nr] = got[0][r0:r0 + nr], got[1][:, r0:r0 + nr]
                    got_cand[a:a + nr], got_count[a:a + nr], got_peak[a:a + nr] = got[2][r0:r0 + nr], got[3][r0:r0 + nr], got[4][r0:r0 + nr]
                    pos[k] = min(pos[k] + P, lens[k])
            t += 1
        assert [pool.info(k)[1] for k in range(n)] == frames
        tk.free()
    o0.free()
    assert most > 256
    assert np.array_equal(_u64(got_rec[:, 2:width]), _u64(want[0][:, 2:width])), "records"
    assert np.array_equal(got_st, want[1]), "status3"
    assert np.array_equal(got_count, want[3]) and np.array_equal(_u64(got_peak), _u64(want[4]))
    keep = np.arange(KMAX)[None, :] < got_count[:, None]
    assert np.array_equal(_u64(got_cand)[keep], _u64(want[2])[keep]), "candidate lists"


# ---- 6. the device form, host memory kinds, foreign calls, policies ---------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["pcm16", "pcm24", "alaw"])
def test_push_device_equals_push(vb, pkg, base, fmt):
    streams = _streams(base, fmt, SMALL, 5)
    devs = [vb.to_device(np.ascontiguousarray(s[0]).view(np.uint8), np.uint8) for s in streams]
    sb = {"pcm16": 2, "pcm24": 3, "alaw": 1}[fmt]
    pos = [0] * 5

    def pusher(pool, entries, kw):
        ents = []
        for k, _, sz in entries:
            ents.append((k, devs[k].ptr + pos[k] * sb, sz))
            pos[k] += sz
        return pool.push_device(ents, **kw)
    _check(vb, pkg, base, fmt, SMALL, "tracked_ext", pusher=pusher, resident=False)
    vb.sync()
    for d in devs:
        d.free()


def test_pinned_blocks_overwritten_when_the_push_returns(vb, pkg, base):
    """the host form returns when every block has been read: one pinned buffer per stream, refilled for every tick with no wait"""
    N, H = SMALL
    stage = [vb.malloc_host((N + 80 * H,), np.int16) for _ in range(5)]

    def pusher(pool, entries, kw):
        ents = []
        for k, blk, sz in entries:
            stage[k][:sz] = blk
            ents.append((k, stage[k][:sz]))
        r = pool.push(ents, **kw)
        for k, _, sz in entries:
            stage[k][:sz] = -12345
        return r
    _check(vb, pkg, base, "pcm16", SMALL, "tracked_ext", pusher=pusher, resident=False)
    vb.sync()
    for s in stage:
        vb.free_host(s)


def test_foreign_calls_and_a_session_between_ticks(vb, pkg, base):
    """other entry points and a one-channel session's pushes on the same context between the ticks change nothing"""
    other = np.ascontiguousarray(base[:40_000])
    ext, track = ah._form(pkg, "tracked_ext")
    side = _streams(base, "pcm16", SMALL, 6)[5][0]
    sess = _open_sess(vb, pkg, "pcm16", SMALL, "tracked_ext", 4000)
    state = dict(pos=0)

    def between(i):
        if i % 3 == 0:
            vb.analyze_frames(other, ah._params(pkg), frame_len=512, stride=256)
        if i % 4 == 1 and state["pos"] + 900 <= side.size:
            sess.push(side[state["pos"]:state["pos"] + 900])
            state["pos"] += 900
        if i % 7 == 2:
            vb.analyze_host(other, ah._params(pkg), ext, track, chunk_frames=64, seg_start=[0, 20], frame_len=1024, stride=512)
    _check(vb, pkg, base, "pcm16", SMALL, "tracked_ext", between=between, resident=False)
    sess.close()


def test_lpc_policy_reference(vb, pkg, base, request):
    old = vb.lpc_policy
    request.addfinalizer(lambda: setattr(vb, "lpc_policy", old))
    vb.lpc_policy = pkg.LPC_POLICY_REFERENCE
    _check(vb, pkg, base, "pcm16", SMALL, "plain", policy="REFERENCE")


# ---- 7. ticks without rows; 8. rejections ----------------------------------------------------------------------------------------

def test_zero_row_ticks_write_nothing_and_rejections_leave_the_pool_usable(vb, pkg, base):
    form, fmt, shape = "tracked_ext", "pcm16", SMALL
    N, H = shape
    streams = _streams(base, fmt, shape, 3)
    L = vb.L
    o0 = gs.Outputs(vb, pkg, form)
    ext, track = ah._form(pkg, form)
    p = ah._params(pkg)
    hf = pkg.HostAudio.make(1, 1, 0, 0)
    h = C.c_void_p()

    def open_(fmt_=hf, n=N, s=H, ms=3, mb=N + 80 * H, mt=3 * (N + 80 * H), par=p):
        rc = L.vbx_pool_open(vb.ctx, None if fmt_ is None else C.byref(fmt_), n, s, None if par is None else C.byref(par), C.byref(ext), C.byref(track),
                             ms, mb, mt, C.byref(h))
        assert rc != 0 or h.value
        return rc
    for bad in (dict(fmt_=None), dict(par=None), dict(fmt_=pkg.HostAudio.make(1, 2, 0, 0)), dict(fmt_=pkg.HostAudio.make(1, 1, 0, 5)),
                dict(fmt_=pkg.HostAudio.make(9, 1, 0, 0)), dict(n=4097, s=2048), dict(n=0), dict(s=0), dict(ms=0), dict(mb=0), dict(mt=10),
                dict(ms=1 << 26, mt=1 << 40)):
        assert open_(**bad) == E_INVALID and not h.value, bad
    assert L.vbx_pool_open(vb.ctx, C.byref(hf), N, H, C.byref(p), None, None, 3, 100, 300, None) == E_INVALID
    with _open_pool(vb, pkg, fmt, shape, form, 3, N + 80 * H) as pool:
        tk = Tick(vb, o0, 100)
        tk.clear()
        kw = tk.kw()
        # ticks that complete no frame: sub-frame blocks, empty blocks, no entries at all -- nothing is written, the samples are carried
        for ents in ([], [(0, streams[0][0][:1]), (2, streams[2][0][:7])], [(1, streams[1][0][:0])], [(0, streams[0][0][1:N - 1]), (1, streams[1][0][:5])]):
            rows, total = pool.push(ents, **kw)
            assert total == 0 and all(r[1] == 0 for r in rows)
        tk.download(0)
        assert pool.info(0)[:2] == (N - 1, 0) and pool.info(2)[:2] == (7, 0) and pool.info(1)[:2] == (5, 0)
        # rejections: each leaves the pool's state unchanged
        before = [pool.info(k) for k in range(3)]
        blk = np.ascontiguousarray(streams[0][0][N - 1:N - 1 + 4 * H])
        dev = vb.to_device(streams[0][0][:4 * H + 8], np.int16)
        E = pkg.PoolEntry
        rows_out = (pkg.PoolRows * 4)()
        tot = C.c_size_t(77)
        po = pkg.PitchTrackOutputs(tk.lists[0].ptr, tk.lists[1].ptr, tk.lists[2].ptr, None)
        good = dict(ents=[E(0, blk.ctypes.data, 4 * H)], rec=tk.rec.ptr, ld=o0.ld, st=tk.st.ptr, st_ld=tk.n, po=po, device=False)

        def push(**over):
            a = dict(good, **over)
            arr = (E * max(len(a["ents"]), 1))(*a["ents"]) if a["ents"] is not None else None
            fn = L.vbx_pool_push_device if a["device"] else L.vbx_pool_push
            return fn(pool.handle, arr, len(a["ents"]) if a["ents"] is not None else 2, a["rec"], a["ld"], a["st"], a["st_ld"],
                      None if a["po"] is None else C.byref(a["po"]), rows_out, C.byref(tot))
        big = np.zeros(N + 81 * H, np.int16)
        cases = [dict(ents=None), dict(ents=[E(3, blk.ctypes.data, 4 * H)]), dict(ents=[E(-1, blk.ctypes.data, 4 * H)]),
                 dict(ents=[E(0, blk.ctypes.data, 4 * H), E(0, blk.ctypes.data, H)]), dict(ents=[E(0, None, 4 * H)]),
                 dict(ents=[E(0, big.ctypes.data, big.size)]), dict(ents=[E(0, dev.ptr + 1, 4 * H)], device=True),
                 dict(rec=None), dict(rec=tk.rec.ptr + 8), dict(ld=o0.ld - 1), dict(ld=o0.width - 2), dict(st_ld=3), dict(po=None),
                 dict(po=pkg.PitchTrackOutputs(None, tk.lists[1].ptr, tk.lists[2].ptr, None)),
                 dict(po=pkg.PitchTrackOutputs(tk.lists[0].ptr, tk.lists[1].ptr, None, None)),
                 dict(po=pkg.PitchTrackOutputs(tk.lists[0].ptr, tk.lists[1].ptr, tk.lists[2].ptr, tk.lists[1].ptr))]
        for bad in cases:
            assert push(**bad) == E_INVALID, bad
            assert [pool.info(k) for k in range(3)] == before, bad
        assert L.vbx_pool_push(None, None, 0, None, 0, None, 0, None, None, None) == E_INVALID
        assert L.vbx_pool_mark_utterance(pool.handle, 3) == E_INVALID and L.vbx_pool_reset_stream(pool.handle, -1) == E_INVALID
        assert L.vbx_pool_info(pool.handle, 5, None, None, None) == E_INVALID
        # a tick of more than max_tick samples in all (every block within max_block)
        with _open_pool(vb, pkg, fmt, shape, form, 3, 2 * H, max_tick=3 * H) as small:
            e3 = [E(k, blk.ctypes.data, 2 * H) for k in range(3)][:2]
            arr = (E * 2)(*e3)
            assert L.vbx_pool_push(small.handle, arr, 2, tk.rec.ptr, o0.ld, tk.st.ptr, tk.n, C.byref(po), None, None) == E_INVALID
            assert small.info(0)[0] == 0 and small.info(1)[0] == 0
        tk.download(0)                                                            # nothing was written by any of them
        dev.free()
        # ... and the pool goes on: the next tick's output equals the session's
        assert push() == 0 and tot.value == 4 and (rows_out[0].row_start, rows_out[0].n_rows) == (0, 4)
        got = tk.download(4)
        tk.free()
    o = gs.Outputs(vb, pkg, form, 4)
    with _open_sess(vb, pkg, fmt, shape, form, N + 4 * H) as sess:
        sess.push(streams[0][0][:N - 1 + 4 * H], **o.at(0))
    want = o.download()
    o.free()
    _same("the tick after the rejections", tuple(a[..., :4] if a.ndim == 2 and a.shape[0] == 3 else a[:4] for a in got), want)
    o0.free()


# ---- 9. launches do not depend on the entry count -----------------------------------------------------------------------------------

def test_launches_do_not_depend_on_the_entry_count(vb, pkg, base):
    """one steady-state tick (1200/480 PCM16, tracked_ext, every stream past warm = 64) with 1, 3 and 40 entries: the same launches"""
    N, H = NATIVE
    form = "tracked_ext"
    streams = _streams(base, "pcm16", NATIVE, 5)
    o0 = gs.Outputs(vb, pkg, form)
    reports = {}
    for n in (1, 3, 40):
        with _open_pool(vb, pkg, "pcm16", NATIVE, form, n, N + 79 * H) as pool:
            tk = Tick(vb, o0, 82 * n)
            pos = 0
            for sz in (N + 79 * H, H, H):
                tk.clear()
                pool.push([(k, streams[k % 5][0][pos + k:pos + k + sz]) for k in range(n)], **tk.kw())
                pos += sz
            assert pkg.session_plan(pos, 0, H, N, H).warm == 64
            vb.sync()
            vb.profile(True)
            vb.profile_reset()
            try:
                rows, total = pool.push([(k, streams[k % 5][0][pos + k:pos + k + H]) for k in range(n)], **tk.kw())
                vb.sync()
                reports[n] = {name: cnt for name, (_, cnt) in vb.profile_report().items()}
            finally:
                vb.profile(False)
            assert total == n
            tk.free()
    o0.free()
    assert reports[1] == reports[3] == reports[40], reports
    rep = reports[40]
    assert rep["pool_ingest_pcm16"] == 1 and rep["tracker_stitch_pool"] == 1 and rep["pool_deliver"] == 1, rep
    assert not [name for name in rep if name.startswith("session_")], rep
    assert "pcm16" not in rep                                                     # 1200-sample PCM16 frames are read without a widening pass
