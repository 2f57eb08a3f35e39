"""vbx_session_path_bind_channels on a real MI355X: the pitch contour of EVERY channel of a multi-channel live session, committed by one
launch per push.  The yardstick is n_sel bound ONE-channel sessions (vbx_session_path_bind, tests/test_gpu_session_path.py) on the same
context, pushed the same blocks: per channel the committed rows, indices, forced flags and commit records must be equal push by push
-- every push and every mark writes into a slot of its own of canary-filled arrays, so the arrays are compared byte for byte -- and
so must everything else a push writes.  The recording is the five-channel one of tests/test_gpu_session_channels.py."""
import numpy as np
import pytest

import test_gpu_session_channels as sc
import test_gpu_session_path as sp
from test_gpu_session import base  # noqa: F401  (the module-scoped recording fixture)

pytestmark = pytest.mark.gpu

F, N, H = sp.F, 1200, 480
SEL = sc.SEL
MARKS = (61, 140)
# pushes end exactly where the frame count reaches 61 and 140; hops, a push that completes no frame, large blocks
SIZES = [N + 60 * H] + [H] * 19 + [7, H - 7] + [59 * H] + [H] * 10 + [50 * H]
assert sum(SIZES) == (F - 1) * H + N


def _bind_all(sess, runs, slot, peak_ref, mp):
    r = slot * runs[0].rows
    sess.bind_path([x.path.ptr + 16 * r for x in runs], [x.commit.ptr + 32 * slot for x in runs], peak_ref=peak_ref, max_pending=mp,
                   out_index=[x.index.ptr + 4 * r for x in runs], out_forced=[x.forced.ptr + r for x in runs])


def _feed(sess, runs, audio, sizes, marks, peak_ref, mp, multi, bound=True):
    """every push and every mark gets the next slot of the bound arrays; the stream ends with a mark; returns the slots used"""
    pos, slot, done = 0, 0, set()

    def bind():
        nonlocal slot
        if bound:
            if multi:
                _bind_all(sess, runs, slot, peak_ref, mp)
            else:
                runs[0].bind(sess, slot, peak_ref=peak_ref, mp=mp)
            slot += 1
    for n in sizes:
        lo = sess.info()[1]
        if lo in marks and lo not in done:
            done.add(lo)
            bind()
            sess.mark_utterance()
        bind()
        if multi:
            at = [x.push_args(lo) for x in runs]
            kw = dict(out=[a["out"] for a in at], status=[a["status"] for a in at], outputs=[a["outputs"] for a in at],
                      record_ld=at[0]["record_ld"], status_ld=at[0]["status_ld"])
        else:
            kw = runs[0].push_args(lo)
        assert sess.push(audio[pos:pos + n], **kw) is None
        pos += n
    bind()
    sess.mark_utterance()                                      # the rest of every channel's contour, at once
    return slot


def _track(pkg, kmax, silence):
    return pkg.PitchTrackParams.make(kmax=kmax, silence_threshold=silence)


def _pair(vb, pkg, base, kmax, silence, mp, fmt="pcm16", sel=SEL, sizes=SIZES, marks=MARKS, peak_ref=1.0):
    """(the multi-channel session's arrays per channel, the one-channel sessions' arrays per channel, slots used)"""
    audio = sc._recording(base, fmt, 5, (N, H))[0]
    n_slots = len(sizes) + len(marks) + 1
    rows = mp + max(sizes) // H + 2
    p, track = sp._params(pkg), _track(pkg, kmax, silence)
    runs = [sp.Run(vb, pkg, kmax, n_slots, rows) for _ in sel]
    ones = [sp.Run(vb, pkg, kmax, n_slots, rows) for _ in sel]
    try:
        with vb.session_channels(p, None, track, format=sc.CODE[fmt], channels=5, select=sel, frame_len=N, stride=H, max_block=max(sizes)) as sess:
            slots = _feed(sess, runs, audio, sizes, marks, peak_ref, mp, multi=True)
            assert sess.info()[1] == F
        for k, c in enumerate(sel):
            with vb.session(p, None, track, format=sc.CODE[fmt], channels=5, channel=c, frame_len=N, stride=H, max_block=max(sizes)) as one:
                assert _feed(one, [ones[k]], audio, sizes, marks, peak_ref, mp, multi=False) == slots
        vb.sync()
        return [[d.numpy() for d in x.all] for x in runs], [[d.numpy() for d in x.all] for x in ones], slots
    finally:
        for x in runs + ones:
            x.free()


def _assert_equal(label, got, want, sel):
    names = ("records", "status3", "cand", "count", "peak", "path", "index", "forced", "commit")
    for k, c in enumerate(sel):
        for name, a, b in zip(names, got[k], want[k]):
            assert a.tobytes() == b.tobytes(), (label, "channel", c, name)


@pytest.mark.parametrize("silence", [0.0, 0.03])
@pytest.mark.parametrize("kmax", [4, 15])
def test_bound_channels_equal_bound_one_channel_sessions(vb, pkg, base, kmax, silence):
    got, want, slots = _pair(vb, pkg, base, kmax, silence, sp.MP)
    _assert_equal(f"kmax {kmax} silence {silence}", got, want, SEL)
    for k in range(len(SEL)):
        cm = want[k][8][:slots]
        assert int(cm[:, 1].sum()) == F and int(cm[-1, 3]) == 0 and not want[k][7][want[k][7] != 0xFF].any()      # all rows committed, none forced
        # the marks deliver the rest of the channel's contour at the mark: nothing is pending behind one
        mark_slots = [i for i in range(slots) if i > 0 and int(cm[i, 0]) + int(cm[i, 1]) in MARKS + (F,) and int(cm[i, 3]) == 0]
        assert len(mark_slots) >= 3
    assert got[0][5].tobytes() != got[1][5].tobytes()                              # (the channels' contours differ: no plane mix-up can pass)


def test_forced_rows_are_the_references_forced_rows(vb, pkg, base):
    """a cap so small that the one-channel reference itself has to force rows: checked on the reference, then held equal"""
    got, want, slots = _pair(vb, pkg, base, 15, 0.0, 3)
    forced_on = [k for k in range(len(SEL)) if int(want[k][8][:slots, 2].sum()) > 0]
    assert forced_on, "the reference forces no row at this cap: the case is vacuous"
    for k in forced_on:
        flags = want[k][7]
        assert (flags == 1).any()
    _assert_equal("max_pending 3", got, want, SEL)


def test_reset_drops_the_binding(vb, pkg, base):
    audio = sc._recording(base, "pcm16", 5, (N, H))[0]
    n_sf = (50 - 1) * H + N
    kmax = 4
    runs = [sp.Run(vb, pkg, kmax, 4, sp.MP + 60) for _ in SEL]
    p, track = sp._params(pkg), _track(pkg, kmax, 0.0)
    L = vb.L

    def push(sess):
        at = [x.push_args(0) for x in runs]
        sess.push(audio[:n_sf], out=[a["out"] for a in at], status=[a["status"] for a in at], outputs=[a["outputs"] for a in at],
                  record_ld=at[0]["record_ld"], status_ld=at[0]["status_ld"])
    try:
        with vb.session_channels(p, None, track, format=1, channels=5, select=SEL, frame_len=N, stride=H, max_block=n_sf) as sess:
            _bind_all(sess, runs, 0, 1.0, sp.MP)
            push(sess)
            ent = (pkg.ChannelPathOutputs * 3)()
            for k, x in enumerate(runs):
                ent[k].out_path, ent[k].d_commit = x.path.ptr + 16 * x.rows, x.commit.ptr + 32
            # bound: the destinations may change, peak_ref and max_pending may not
            assert L.vbx_session_path_bind_channels(sess.handle, 1.0, sp.MP + 1, ent, 2) == -1
            assert L.vbx_session_path_bind_channels(sess.handle, 0.5, sp.MP, ent, 2) == -1
            sess.reset()
            push(sess)                                           # unbound again: slot 1 stays untouched
            assert L.vbx_session_path_bind_channels(sess.handle, 1.0, sp.MP, ent, 2) == -1         # not mid-stream
            sess.reset()
            _bind_all(sess, runs, 2, 1.0, 32)                    # a new binding may choose anew
            push(sess)
            _bind_all(sess, runs, 3, 1.0, 32)
            sess.mark_utterance()
            vb.sync()
            for x in runs:
                cm = x.commit.numpy()
                r = x.rows
                assert np.all(cm[1] == -1) and np.all(sp._u64(x.path.numpy()[r:2 * r]) == 0xFFFFFFFFFFFFFFFF)
                assert cm[2][0] == 0 and cm[2][1] + cm[2][3] == 50 and tuple(cm[3]) == (cm[2][1], cm[2][3], 0, 0)      # counted from the reset
                assert cm[0][1] == cm[2][1]                      # the same frames, the same decisions
    finally:
        for x in runs:
            x.free()


def test_one_path_launch_per_push(vb, pkg, base):
    """the online path's name is launched exactly once per push, for one selected channel and for five"""
    audio = sc._recording(base, "pcm16", 5, (N, H))[0]
    kmax = 4
    p, track = sp._params(pkg), _track(pkg, kmax, 0.0)
    for sel in ([2], [4, 0, 2, 1, 3]):
        runs = [sp.Run(vb, pkg, kmax, 3, sp.MP + 90) for _ in sel]
        try:
            with vb.session_channels(p, None, track, format=1, channels=5, select=sel, frame_len=N, stride=H, max_block=N + 79 * H) as sess:
                def push(a, b, lo, slot):
                    _bind_all(sess, runs, slot, 1.0, sp.MP)
                    at = [x.push_args(lo) for x in runs]
                    sess.push(audio[a:b], out=[q["out"] for q in at], status=[q["status"] for q in at], outputs=[q["outputs"] for q in at],
                              record_ld=at[0]["record_ld"], status_ld=at[0]["status_ld"])
                push(0, N + 79 * H, 0, 0)
                vb.sync()
                vb.profile(True)
                vb.profile_reset()
                try:
                    push(N + 79 * H, N + 80 * H, 80, 1)
                    vb.sync()
                    rep = {name: cnt for name, (_, cnt) in vb.profile_report().items()}
                finally:
                    vb.profile(False)
                assert rep.get("pitch_path_online_all") == 1 and "pitch_path_online" not in rep, (sel, rep)
                assert rep["session_deliver_all"] == 1 and rep["session_ingest_all_pcm16"] == 1, (sel, rep)
        finally:
            for x in runs:
                x.free()


def test_rejections(vb, pkg, base):
    L = vb.L
    path, commit = vb.empty((3, sp.MP + 8, 2)), vb.empty((3, 4), np.int64)
    p = sp._params(pkg)

    def entries(n=3, no_path=None, no_commit=None):
        ent = (pkg.ChannelPathOutputs * n)()
        for k in range(n):
            ent[k].out_path = None if k == no_path else path.ptr + k * (sp.MP + 8) * 16
            ent[k].d_commit = None if k == no_commit else commit.ptr + k * 32
        return ent
    try:
        assert L.vbx_session_path_bind_channels(None, 1.0, sp.MP, entries(), 2) == -1                       # NULL session
        with vb.session(p, None, _track(pkg, 4, 0.0), format=1, channels=5, channel=0, frame_len=N, stride=H, max_block=N) as one:
            assert L.vbx_session_path_bind_channels(one.handle, 1.0, sp.MP, entries(), 2) == -1             # a one-channel session
        with vb.session_channels(p, None, None, format=1, channels=5, select=SEL, frame_len=N, stride=H, max_block=N) as plain:
            assert L.vbx_session_path_bind_channels(plain.handle, 1.0, sp.MP, entries(), 2) == -1           # no h_track: no lists
        with vb.session_channels(p, None, _track(pkg, 4, 0.03), format=1, channels=5, select=SEL, frame_len=N, stride=H, max_block=N) as sess:
            bind = lambda ent=entries(), peak=1.0, mp=sp.MP, ld=2: L.vbx_session_path_bind_channels(sess.handle, peak, mp, ent, ld)
            assert bind(ent=None) == -1 and bind(ent=entries(no_path=1)) == -1 and bind(ent=entries(no_commit=2)) == -1
            assert bind(ld=1) == -1 and bind(mp=0) == -1
            for peak in (-1.0, float("nan"), float("inf")):                                                 # silence > 0 needs a usable peak_ref
                assert bind(peak=peak) == -1
            assert bind() == 0 and bind() == 0                                                              # ... and the session is still usable
    finally:
        path.free(); commit.free()
