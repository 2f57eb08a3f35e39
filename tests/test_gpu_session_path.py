"""vbx_session_path_bind: the pitch contour from a live session while the audio arrives (include/voxbox_hip.h).

With silence_threshold == 0 and no forced row, the rows all pushes commit, concatenated, are columns 0-1 and `index` of the resident
tracked call on the concatenated blocks, bit for bit, for every way of cutting the audio into blocks; everything else a push
writes is what an unbound session writes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 48000.0
F = 200
MP = 64
i32, i64, u8 = np.int32, np.int64, np.uint8
_REF, _AUDIO = {}, {}


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _params(pkg):
    return pkg.AnalysisParams.make(SR, est_init=np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES]))


def _track(pkg, kmax, silence=0.0):
    return pkg.PitchTrackParams.make(kmax=kmax, silence_threshold=silence)


def _audio(vb, fmt, N, H):
    """(host audio in the session's type, format code)"""
    if (fmt, N, H) not in _AUDIO:
        if "x" not in _AUDIO:
            d = vb.synth_speech((F - 1) * 1000 + 1200, sample_offset=7 * 48000 + 99)
            _AUDIO["x"] = d.numpy() * 0.9
            d.free()
        x = _AUDIO["x"][:(F - 1) * H + N]
        _AUDIO[(fmt, N, H)] = (np.round(x * 32767.0).astype(np.int16), 1) if fmt == "pcm16" else (x.copy(), 5)
    return _AUDIO[(fmt, N, H)]


def _resident(vb, pkg, fmt, N, H, kmax, seg=None, silence=0.0):
    key = (fmt, N, H, kmax, None if seg is None else tuple(seg), silence)
    if key not in _REF:
        audio, _ = _audio(vb, fmt, N, H)
        fn = vb.analyze_frames_ex_pcm16 if fmt == "pcm16" else vb.analyze_frames_ex
        _REF[key] = fn(audio, _params(pkg), None, _track(pkg, kmax, silence), seg_start=None if seg is None else np.asarray(seg, i64),
                       frame_len=N, stride=H, n_frames=F, lists=True)
    return _REF[key]


def _schedule(name, N, H):
    T = (F - 1) * H + N
    if name == "one":
        return [T]
    if name == "hop":
        return [N] + [H] * (F - 1)
    step = H // 3                                              # sub-hop: two of three pushes complete no frame
    return [step] * (T // step) + ([T % step] if T % step else [])


class Run:
    """a session's global outputs (canary-filled) and, per push, its own rows of the bound arrays and its own commit record"""

    def __init__(self, vb, pkg, kmax, n_pushes, rows_per_push):
        self.vb, self.kmax, self.rows = vb, kmax, rows_per_push
        p = _params(pkg)
        self.width = int(vb.L.vbx_record_doubles_ex(C.byref(p), None))
        self.ld = self.width + (self.width & 1)
        self.rec, self.st = vb.empty((F, self.ld)), vb.empty((3, F), i32)
        self.lists = [vb.empty((F, kmax, 2)), vb.empty(F, i32), vb.empty(F)]
        tot = n_pushes * rows_per_push
        self.path, self.index, self.forced, self.commit = vb.empty((tot, 2)), vb.empty(tot, i32), vb.empty(tot, u8), vb.empty((n_pushes, 4), i64)
        self.all = [self.rec, self.st] + self.lists + [self.path, self.index, self.forced, self.commit]
        for d in self.all:
            vb._check(vb.L.vbx_memset(vb.ctx, d.ptr, 0xFF, d.nbytes))

    def push_args(self, lo):
        outs = (self.lists[0].ptr + lo * self.kmax * 16, self.lists[1].ptr + lo * 4, self.lists[2].ptr + lo * 8, None)
        return dict(out=self.rec.ptr + lo * self.ld * 8, status=self.st.ptr + lo * 4, outputs=outs, record_ld=self.ld, status_ld=F)

    def bind(self, sess, i, peak_ref=1.0, mp=MP):
        r = i * self.rows
        sess.bind_path(self.path.ptr + 16 * r, self.commit.ptr + 32 * i, peak_ref=peak_ref, max_pending=mp,
                       out_index=self.index.ptr + 4 * r, out_forced=self.forced.ptr + r)

    def contour(self, n_used):
        """the committed rows of slots [0, n_used), concatenated, and the commit records; rows beyond n are untouched"""
        self.vb.sync()
        p, ix, fo, cm = self.path.numpy(), self.index.numpy(), self.forced.numpy(), self.commit.numpy()
        gp, gi, gf = [np.empty((0, 2))], [np.empty(0, i32)], [np.empty(0, u8)]
        for i in range(n_used):
            n, a = int(cm[i, 1]), i * self.rows
            assert 0 <= n <= self.rows, (i, cm[i])
            gp.append(p[a:a + n]); gi.append(ix[a:a + n]); gf.append(fo[a:a + n])
            assert np.all(_u64(p[a + n:a + self.rows]) == 0xFFFFFFFFFFFFFFFF) and np.all(fo[a + n:a + self.rows] == 0xFF), i
        return np.concatenate(gp), np.concatenate(gi), np.concatenate(gf), [tuple(int(v) for v in c) for c in cm[:n_used]]

    def free(self):
        for d in self.all:
            d.free()


def _feed(sess, run, audio, sizes, marks=(), bound=True, slot0=0):
    """every push (and every mark) gets the next slot of the bound arrays; returns the slots used"""
    pos, slot, done = 0, slot0, set()
    for n in sizes:
        lo = sess.info()[1]
        if lo in marks and lo not in done:
            done.add(lo)
            if bound:
                run.bind(sess, slot)
                slot += 1
            sess.mark_utterance()
        if bound:
            run.bind(sess, slot)
            slot += 1
        assert sess.push(audio[pos:pos + n], **run.push_args(lo)) is None
        pos += n
    return slot



def _open(vb, pkg, fmt, code, N, H, kmax, max_block, silence=0.0):
    return vb.session(_params(pkg), None, _track(pkg, kmax, silence), format=code, frame_len=N, stride=H, max_block=max_block)


def _check_contour(vb, pkg, fmt, N, H, kmax, schedule, marks=()):
    audio, code = _audio(vb, fmt, N, H)
    seg = [0] + list(marks) if marks else None
    want = _resident(vb, pkg, fmt, N, H, kmax, seg)
    sizes = _schedule(schedule, N, H)
    nmax = max(sizes) // H + 2
    run = Run(vb, pkg, kmax, len(sizes) + len(marks) + 1, MP + nmax)
    try:
        with _open(vb, pkg, fmt, code, N, H, kmax, max(sizes)) as sess:
            slots = _feed(sess, run, audio, sizes, marks)
            assert sess.info()[1] == F
            run.bind(sess, slots)                              # the stream ends: the mark delivers the rest
            sess.mark_utterance()
            gp, gi, gf, cm = run.contour(slots + 1)
        assert not gf.any()
        assert gp.shape == (F, 2), gp.shape
        a, b = _u64(gp), _u64(want[0][:, :2])
        assert np.array_equal(a, b), (fmt, kmax, schedule, "first differing row", np.argwhere(a != b)[:4])
        assert np.array_equal(gi, want[5])
        first = 0
        for c in cm:                                           # the records chain, and the mark leaves nothing pending
            assert c[0] == first and c[2] == 0 and 0 <= c[3] <= MP
            first += c[1]
        assert cm[-1][3] == 0
        got_rec, got_st = run.rec.numpy(), run.st.numpy()
        assert np.array_equal(_u64(got_rec[:, 2:run.width]), _u64(want[0][:, 2:run.width])) and np.array_equal(got_st, want[1])
        assert np.all(_u64(got_rec[:, :2]) == 0xFFFFFFFFFFFFFFFF)               # columns 0-1 of the records stay the caller's
        return cm
    finally:
        run.free()


@pytest.mark.parametrize("schedule", ["sub-hop", "hop", "one"])
@pytest.mark.parametrize("kmax", [4, 15])
@pytest.mark.parametrize("fmt", ["pcm16", "f64"])
def test_the_committed_rows_are_the_resident_contour(vb, pkg, fmt, kmax, schedule):
    cm = _check_contour(vb, pkg, fmt, 1200, 480, kmax, schedule)
    if schedule == "hop":                                      # the contour trails the audio by a few frames, not by the utterance
        assert max(c[3] for c in cm) < 32 and sum(1 for c in cm if c[1] > 0) > F // 4


@pytest.mark.parametrize("schedule", ["sub-hop", "hop", "blocks"])
@pytest.mark.parametrize("fmt", ["pcm16", "f64"])
def test_two_marks_are_seg_start(vb, pkg, fmt, schedule):
    marks = (61, 140)
    if schedule == "blocks":                                   # large blocks: three of them, ending where the marked frames begin
        _three_blocks(vb, pkg, fmt, marks)
    else:
        _check_contour(vb, pkg, fmt, 1200, 480, 4, schedule, marks)


def _three_blocks(vb, pkg, fmt, marks):
    """large blocks that end exactly where the marked frames begin"""
    N, H, kmax = 1200, 480, 15
    audio, code = _audio(vb, fmt, N, H)
    want = _resident(vb, pkg, fmt, N, H, kmax, [0] + list(marks))
    T = (F - 1) * H + N
    cuts = [0] + [(m - 1) * H + N for m in marks] + [T]        # frame m - 1 is complete, frame m is not
    sizes = [b - a for a, b in zip(cuts, cuts[1:])]
    run = Run(vb, pkg, kmax, 8, MP + max(sizes) // H + 2)
    try:
        with _open(vb, pkg, fmt, code, N, H, kmax, max(sizes)) as sess:
            slots = _feed(sess, run, audio, sizes, marks)
            run.bind(sess, slots)
            sess.mark_utterance()
            gp, gi, gf, cm = run.contour(slots + 1)
        assert not gf.any() and np.array_equal(_u64(gp), _u64(want[0][:, :2])) and np.array_equal(gi, want[5])
        marks_cm = [cm[1], cm[3], cm[5]]                       # push, mark, push, mark, push, mark
        assert all(c[3] == 0 for c in marks_cm)
    finally:
        run.free()


def test_another_shape(vb, pkg):
    _check_contour(vb, pkg, "f64", 512, 512, 4, "hop")
    _check_contour(vb, pkg, "pcm16", 512, 512, 15, "sub-hop", marks=(77,))


def test_the_mark_delivers_the_rest_at_once(vb, pkg):
    N, H, kmax = 1200, 480, 15
    audio, code = _audio(vb, "pcm16", N, H)
    want = _resident(vb, pkg, "pcm16", N, H, kmax, [0, 120])
    n_sf = (120 - 1) * H + N                                   # 120 frames, in one block
    run = Run(vb, pkg, kmax, 3, MP + 130)
    try:
        with _open(vb, pkg, "pcm16", code, N, H, kmax, n_sf) as sess:
            run.bind(sess, 0)
            sess.push(audio[:n_sf], **run.push_args(0))
            run.bind(sess, 1)
            sess.mark_utterance()                              # no frame arrives behind it
            gp, gi, gf, cm = run.contour(2)
        assert cm[0][0] == 0 and cm[0][1] + cm[0][3] == 120
        assert cm[1] == (cm[0][1], cm[0][3], 0, 0)
        assert np.array_equal(_u64(gp), _u64(want[0][:120, :2])) and np.array_equal(gi, want[5][:120]) and not gf.any()
    finally:
        run.free()


def test_the_rest_of_a_push_is_an_unbound_sessions(vb, pkg):
    """records from column 2, status rows and h_outputs: bit for bit what the same pushes write without a binding (silence > 0, so
    the peaks are delivered too; peak_ref is then the path's P and the bound rows differ from nothing the unbound session writes)"""
    N, H, kmax = 1200, 480, 4
    audio, code = _audio(vb, "pcm16", N, H)
    sizes = _schedule("sub-hop", N, H)[:240] + [(F - 1) * H + N - sum(_schedule("sub-hop", N, H)[:240])]
    got = []
    for bound in (False, True):
        run = Run(vb, pkg, kmax, len(sizes) + 1, MP + max(sizes) // H + 2)
        try:
            with _open(vb, pkg, "pcm16", code, N, H, kmax, max(sizes), silence=0.03) as sess:
                slots = _feed(sess, run, audio, sizes, bound=bound)
                vb.sync()
                got.append([d.numpy() for d in [run.rec, run.st] + run.lists])
                if bound:
                    _, _, _, cm = run.contour(slots)
                    assert sum(c[1] for c in cm) + cm[-1][3] == F
                else:
                    assert np.all(run.commit.numpy() == -1)    # nothing of the path's was written
        finally:
            run.free()
    for a, b in zip(*got):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("schedule", ["sub-hop", "hop", "one"])
@pytest.mark.parametrize("fmt", ["pcm16", "f64"])
def test_with_a_silence_threshold_the_rows_are_the_shard_protocols(vb, pkg, fmt, schedule):
    """silence_threshold > 0: the committed rows equal the world-1 shard calls over the session's lists with every utterance's
    seg_peak = peak_ref (two utterances: one mark)"""
    N, H, kmax, peak_ref, mark, SIL = 1200, 480, 4, 0.8, 90, 0.5     # (a threshold at which the synthetic speech has frames that count as quiet)
    audio, code = _audio(vb, fmt, N, H)
    want = _resident(vb, pkg, fmt, N, H, kmax, [0, mark], silence=SIL)       # its lists, counts, status rows and peaks
    par = pkg.PitchPathParams.make(time_step=H / SR, silence_threshold=SIL)
    seg = np.array([0, mark], i64)
    tmp = [vb.to_device(np.ascontiguousarray(want[2])), vb.to_device(want[3]), vb.to_device(np.ascontiguousarray(want[1][0])), vb.to_device(want[4]),
           vb.to_device(np.array([peak_ref, peak_ref])), vb.empty(64), vb.empty(64, i32), vb.empty(1, i32), vb.empty((F, 2)), vb.empty(F, i32)]
    c, k, st, pk, sp, state, back, changed, path, index = tmp
    sizes = _schedule(schedule, N, H)
    if schedule == "one":                                      # two blocks: the first ends where the marked frame begins
        sizes = [(mark - 1) * H + N, sizes[0] - ((mark - 1) * H + N)]
    run = Run(vb, pkg, kmax, len(sizes) + 3, MP + max(sizes) // H + 2)
    try:
        vb.pitch_path_shard_begin(c, k, st, F, kmax, pk, sp, seg, par, 0, False, False)
        vb.pitch_path_shard_enter(None, state, back, changed)
        vb.pitch_path_shard_finish(None, path, 2, index)
        want_p, want_i = path.numpy(), index.numpy()
        with _open(vb, pkg, fmt, code, N, H, kmax, max(sizes), silence=SIL) as sess:
            pos, slot, marked = 0, 0, False
            for n in sizes:
                lo = sess.info()[1]
                if lo == mark and not marked:
                    marked = True
                    run.bind(sess, slot, peak_ref=peak_ref)
                    slot += 1
                    sess.mark_utterance()
                run.bind(sess, slot, peak_ref=peak_ref)
                slot += 1
                assert sess.push(audio[pos:pos + n], **run.push_args(lo)) is None
                pos += n
            assert marked and sess.info()[1] == F
            run.bind(sess, slot, peak_ref=peak_ref)
            sess.mark_utterance()
            gp, gi, gf, cm = run.contour(slot + 1)
        assert not gf.any() and gp.shape == (F, 2)
        assert np.array_equal(_u64(gp), _u64(want_p)) and np.array_equal(gi, want_i)
        assert np.any(want_p[:, 1][want_p[:, 0] == 0.0] > par.voicing_threshold)           # the silence term is at work
    finally:
        run.free()
        for d in tmp:
            d.free()


def test_reset_drops_the_binding_and_rebinding_starts_over(vb, pkg):
    N, H, kmax = 1200, 480, 4
    audio, code = _audio(vb, "f64", N, H)
    want = _resident(vb, pkg, "f64", N, H, kmax)
    n_sf = (50 - 1) * H + N
    run = Run(vb, pkg, kmax, 6, MP + 60)
    L = vb.L
    try:
        with _open(vb, pkg, "f64", code, N, H, kmax, n_sf) as sess:
            run.bind(sess, 0)
            sess.push(audio[:n_sf], **run.push_args(0))
            # bound: the destinations may change, peak_ref and max_pending may not
            r = run.rows
            assert L.vbx_session_path_bind(sess.handle, 1.0, MP + 1, run.path.ptr + 16 * r, 2, None, None, run.commit.ptr + 32) == -1
            assert L.vbx_session_path_bind(sess.handle, 0.5, MP, run.path.ptr + 16 * r, 2, None, None, run.commit.ptr + 32) == -1
            sess.reset()
            sess.push(audio[:n_sf], **run.push_args(0))        # unbound again: slot 1 stays untouched
            assert L.vbx_session_path_bind(sess.handle, 1.0, MP, run.path.ptr + 16 * r, 2, None, None, run.commit.ptr + 32) == -1   # not mid-stream
            sess.reset()
            run.bind(sess, 2, mp=32)                           # a new binding may choose anew
            sess.push(audio[:n_sf], **run.push_args(0))
            run.bind(sess, 3, mp=32)
            sess.mark_utterance()
            vb.sync()
            cm = run.commit.numpy()
            assert np.all(cm[1] == -1) and np.all(_u64(run.path.numpy()[r:2 * r]) == 0xFFFFFFFFFFFFFFFF)
            assert cm[2][0] == 0 and cm[2][1] + cm[2][3] == 50 and tuple(cm[3]) == (cm[2][1], cm[2][3], 0, 0)      # counted from the reset
            assert cm[0][1] == cm[2][1]                        # the same frames, the same decisions
            p = run.path.numpy()
            got = np.concatenate([p[2 * r:2 * r + cm[2][1]], p[3 * r:3 * r + cm[3][1]]])
            # (an utterance that ends at frame 50 is not the 200-frame one's prefix: only what was decided before the mark is)
            k = int(cm[2][1])
            assert np.array_equal(_u64(got[:k]), _u64(want[0][:k, :2]))
            assert np.array_equal(_u64(p[:k]), _u64(want[0][:k, :2]))
    finally:
        run.free()


def test_rejections(vb, pkg):
    N, H = 1200, 480
    audio, code = _audio(vb, "pcm16", N, H)
    L = vb.L
    path, commit = vb.empty((MP + 8, 2)), vb.empty(4, i64)
    try:
        bind = lambda s, peak=1.0, mp=MP, p=path.ptr, ld=2, c=commit.ptr: L.vbx_session_path_bind(s, peak, mp, p, ld, None, None, c)
        assert bind(None) == -1                                                                 # NULL session
        with vb.session(_params(pkg), None, None, format=code, frame_len=N, stride=H, max_block=N) as plain:
            assert bind(plain.handle) == -1                                                     # no h_track: no lists
        with _open(vb, pkg, "pcm16", code, N, H, 4, N, silence=0.03) as sess:
            assert bind(sess.handle, p=None) == -1 and bind(sess.handle, c=None) == -1          # NULL outputs
            assert bind(sess.handle, ld=1) == -1 and bind(sess.handle, mp=0) == -1
            for peak in (-1.0, float("nan"), float("inf")):                                     # silence > 0 needs a usable peak_ref
                assert bind(sess.handle, peak=peak) == -1
            assert bind(sess.handle) == 0 and bind(sess.handle) == 0                            # ... and the session is still usable
    finally:
        path.free(); commit.free()
