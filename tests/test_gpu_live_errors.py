"""The TEXT of every refusal of the live families -- Session, SessionChannels, Pool: open, push, push_device, path_bind /
_bind_channels -- at the small shape the families' own rejection tests use (1200 / 480 PCM16, tracked_ext, blocks of a few hops).
Those tests pin the codes; the three families share one host-side core for their checks (vbx_live.hpp), so what can change
silently is which text a caller reads, its entry-point prefix included.  Every literal below is written out in full.  Refusals are
argument errors: nothing is launched by a refused call, and after each family's refusals one valid push on the same handle returns,
bit for bit, the rows a handle that was never refused anything returns."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_analyze_host as ah

pytestmark = pytest.mark.gpu

N, H, MB = 1200, 480, 4800
FIRST, NEXT = N + 3 * H, 4 * H                                               # two pushes of four frames each
E_INVALID = -1


@pytest.fixture(scope="module")
def pcm(vb):
    d = vb.synth_speech(2 * (FIRST + NEXT), sample_offset=7 * 48000 + 11)
    x = d.numpy()
    d.free()
    return np.round(x * 30000.0).astype(np.int16)


class Refusals:
    """refused(rc, text): the call returned VBX_E_INVALID and left exactly this text (ctx=False: a call without a context or a handle
    leaves it as the thread's last error)"""

    def __init__(self, vb):
        self.vb = vb

    def __call__(self, rc, text, ctx=True):
        got = self.vb.L.vbx_last_error(self.vb.ctx if ctx else None).decode()
        assert rc == E_INVALID and got == text, (rc, got, text)


def _fmt(pkg, format=1, channels=1, channel=0, reserved=0, chunk=0):
    f = pkg.HostAudio.make(format, channels, channel, chunk)
    f.reserved = reserved
    return f


def _bits(rows):
    return [np.ascontiguousarray(a).view(np.uint8).tobytes() for a in rows]


class Bufs:
    """device outputs of 8 rows for one channel, and the lists' struct over them"""

    def __init__(self, vb, pkg, ld):
        self.rec, self.st = vb.empty((8, ld)), vb.empty((3, 8), np.int32)
        self.cand, self.count, self.peak, self.index = vb.empty((8, 4, 2)), vb.empty(8, np.int32), vb.empty(8), vb.empty(8, np.int32)
        self.po = pkg.PitchTrackOutputs(self.cand.ptr, self.count.ptr, self.peak.ptr, None)
        self.path, self.commit = vb.empty((64 + 8, 2)), vb.empty(4)

    def lists(self, pkg, cand=True, count=True, peak=True, index=False):
        return pkg.PitchTrackOutputs(self.cand.ptr if cand else None, self.count.ptr if count else None, self.peak.ptr if peak else None,
                                     self.index.ptr if index else None)

    def free(self):
        for a in (self.rec, self.st, self.cand, self.count, self.peak, self.index, self.path, self.commit):
            a.free()


def _open_texts(refused, opn, fn, pkg):
    """the refusals every open shares, in the words of entry point `fn`; opn(**over) -> rc"""
    refused(opn(out=None), fn + ": null output")
    refused(opn(no_fmt=True), fn + ": null argument")
    refused(opn(no_params=True), fn + ": null argument")
    refused(opn(hf=dict(format=0)), fn + ": unknown sample format")
    refused(opn(hf=dict(format=6)), fn + ": unknown sample format")
    refused(opn(hf=dict(reserved=1)), fn + ": reserved and chunk_frames must be 0")
    refused(opn(hf=dict(chunk=64)), fn + ": reserved and chunk_frames must be 0")
    bad_n = ah._params(pkg)
    bad_n.n_est = 7
    refused(opn(prm=bad_n), fn + ": n_est must be in [1, 6]")
    bad_n.n_est = 0
    refused(opn(prm=bad_n), fn + ": n_est must be in [1, 6]")
    refused(opn(t=pkg.PitchTrackParams.make(kmax=0)), fn + ": kmax must be in [1, 63] (at most 64 states per frame)")
    refused(opn(t=pkg.PitchTrackParams.make(kmax=64)), fn + ": kmax must be in [1, 63] (at most 64 states per frame)")
    # what only the frame loop's parts know: refused by the warm-up call, whose text survives the frees
    refused(opn(e=pkg.AnalysisExt.make(-1.0)), fn + ": resample_ratio must be finite and >= 0")


def test_session_refusal_texts(vb, pkg, pcm):
    L, refused = vb.L, Refusals(vb)
    p = ah._params(pkg)
    ext, track = ah._form(pkg, "tracked_ext")
    h = C.c_void_p()

    def opn(ctx=vb.ctx, hf=None, no_fmt=False, n=N, s=H, prm=p, e=ext, t=track, mb=MB, out=h, no_params=False):
        f = _fmt(pkg, **(hf or {}))
        rc = L.vbx_session_open(ctx, None if no_fmt else C.byref(f), n, s, None if no_params else C.byref(prm), None if e is None else C.byref(e),
                                None if t is None else C.byref(t), mb, None if out is None else C.byref(out))
        assert not h.value
        return rc
    fn = "vbx_session_open"
    refused(opn(ctx=None), fn + ": null context", ctx=False)
    _open_texts(refused, opn, fn, pkg)
    for bad in (dict(channels=0), dict(channels=2, channel=2), dict(channel=-1)):
        refused(opn(hf=bad), fn + ": need channels >= 1 and 0 <= channel < channels")
    refused(opn(mb=0), fn + ": max_block_sample_frames must be >= 1")
    refused(opn(n=0), fn + ": frame_len must be in [1, 67108864]")
    refused(opn(n=67108865), fn + ": frame_len must be in [1, 67108864]")
    refused(opn(s=0), fn + ": stride must be >= 1")
    refused(opn(mb=(1 << 40) + 1), fn + ": max_block_sample_frames or stride too large")
    refused(opn(s=(1 << 40) + 1), fn + ": max_block_sample_frames or stride too large")
    refused(opn(s=1, mb=1 << 31), fn + ": too many frames for one launch")

    ld = ah._width(vb, pkg, "tracked_ext")
    ld += ld & 1
    b = Bufs(vb, pkg, ld)
    dev = vb.to_device(np.zeros(64, np.int16))
    blk = np.ascontiguousarray(pcm[FIRST:FIRST + NEXT])
    with vb.session(p, ext, track, frame_len=N, stride=H, max_block=MB) as sess, \
            vb.session(p, ext, None, frame_len=N, stride=H, max_block=MB) as untracked, \
            vb.session_channels(p, ext, track, channels=2, frame_len=N, stride=H, max_block=MB) as multi:

        def bind(s=sess.handle, peak_ref=1.0, pending=64, path=b.path.ptr, ld_=2, commit=b.commit.ptr):
            return L.vbx_session_path_bind(s, peak_ref, pending, path, ld_, None, None, commit)
        fn = "vbx_session_path_bind"
        refused(bind(s=None), fn + ": null session", ctx=False)
        refused(bind(s=multi.handle), fn + ": the session was opened with vbx_session_open_channels")
        refused(bind(s=untracked.handle), fn + ": the session was opened without h_track: it has no candidate lists")
        refused(bind(path=None), fn + ": null out_path or d_commit")
        refused(bind(commit=None), fn + ": null out_path or d_commit")
        refused(bind(ld_=1), fn + ": path_ld must be >= 2")
        refused(bind(pending=0), fn + ": max_pending must be in [1, 2^24]")
        refused(bind(peak_ref=float("nan")), fn + ": silence_threshold > 0 needs a finite peak_ref >= 0")
        assert bind() == 0
        refused(bind(pending=65), fn + ": a bound session keeps its peak_ref and max_pending (vbx_session_reset drops the binding)")
        refused(bind(peak_ref=2.0), fn + ": a bound session keeps its peak_ref and max_pending (vbx_session_reset drops the binding)")
        sess.reset()                                                         # the binding goes: the pushes below are those of `fresh`
        first = sess.push(pcm[:FIRST])
        refused(bind(), fn + ": bind before the first push or after vbx_session_reset")
        before = sess.info()

        def push(fn_=L.vbx_session_push, s=sess.handle, block=blk.ctypes.data, n=NEXT, rec=b.rec.ptr, rld=ld, st=b.st.ptr, sld=8, po=b.po):
            return fn_(s, block, n, rec, rld, st, sld, None if po is None else C.byref(po), None)
        for fn_, fn, device in ((L.vbx_session_push, "vbx_session_push", False), (L.vbx_session_push_device, "vbx_session_push_device", True)):
            full = dict(fn_=fn_, block=dev.ptr) if device else dict(fn_=fn_)      # (a refused call reads no sample)
            refused(push(fn_=fn_, s=None), fn + ": null session", ctx=False)
            refused(push(fn_=fn_, s=multi.handle), fn + ": the session was opened with vbx_session_open_channels: push with vbx_session_push_channels")
            refused(push(fn_=fn_, block=None), fn + ": null block")
            refused(push(fn_=fn_, n=MB + 1), fn + ": the block is larger than the session's max_block_sample_frames")
            refused(push(rec=None, **full), fn + ": null argument")
            refused(push(rec=b.rec.ptr + 8, **full), fn + ": records must be 16-byte aligned")
            refused(push(rld=ld + 1, **full), fn + ": record_ld must be even and >= vbx_record_doubles(params)")
            refused(push(rld=ld - 2, **full), fn + ": record_ld must be even and >= vbx_record_doubles(params)")
            refused(push(sld=3, **full), fn + ": status_ld must be >= the frames the push delivers")
            refused(push(po=None, **full), fn + ": the tracked form needs h_outputs->cand and ->count")
            refused(push(po=b.lists(pkg, cand=False), **full), fn + ": the tracked form needs h_outputs->cand and ->count")
            refused(push(po=b.lists(pkg, count=False), **full), fn + ": the tracked form needs h_outputs->cand and ->count")
            refused(push(po=b.lists(pkg, peak=False), **full), fn + ": a silence_threshold needs h_outputs->peak")
            refused(push(po=b.lists(pkg, index=True), **full), fn + ": h_outputs->index must be NULL: the caller runs the path (vbx_pitch_path_f64)")
        refused(push(fn_=L.vbx_session_push_device, block=dev.ptr + 1, n=8), "vbx_session_push_device: the block needs its type's alignment")
        assert sess.info() == before and untracked.info() == (0, 0, 0) and multi.info() == (0, 0, 0)
        second = sess.push(blk)
    with vb.session(p, ext, track, frame_len=N, stride=H, max_block=MB) as fresh:
        want = fresh.push(pcm[:FIRST]), fresh.push(blk)
    assert first[0].shape[0] == 4 and second[0].shape[0] == 4
    assert _bits(first) == _bits(want[0]) and _bits(second) == _bits(want[1])
    dev.free()
    b.free()


def test_session_channels_refusal_texts(vb, pkg, pcm):
    L, refused = vb.L, Refusals(vb)
    p = ah._params(pkg)
    ext, track = ah._form(pkg, "tracked_ext")
    h = C.c_void_p()
    sel = np.ascontiguousarray([1, 0], dtype=np.int32)
    audio = np.ascontiguousarray(np.stack([pcm[:FIRST + NEXT], pcm[FIRST + NEXT:]], axis=1))           # [T, 2]

    def opn(ctx=vb.ctx, hf=None, no_fmt=False, sel_=sel, n_sel=2, n=N, s=H, prm=p, e=ext, t=track, mb=MB, out=h, no_params=False):
        f = _fmt(pkg, **dict(dict(channels=2), **(hf or {})))
        rc = L.vbx_session_open_channels(ctx, None if no_fmt else C.byref(f), None if sel_ is None else sel_.ctypes.data, n_sel, n, s,
                                         None if no_params else C.byref(prm), None if e is None else C.byref(e), None if t is None else C.byref(t), mb,
                                         None if out is None else C.byref(out))
        assert not h.value
        return rc
    fn = "vbx_session_open_channels"
    refused(opn(ctx=None), fn + ": null context", ctx=False)
    _open_texts(refused, opn, fn, pkg)
    refused(opn(hf=dict(channels=0)), fn + ": need channels >= 1 and 0 <= channel < channels")
    refused(opn(hf=dict(channel=1)), fn + ": channel must be 0 (the selection is h_channels)")
    selection = fn + ": need 1 <= n_sel <= min(channels, VBX_HOST_MAX_CHANNELS) distinct channels in [0, channels)"
    refused(opn(sel_=None), selection)
    refused(opn(n_sel=0), selection)
    refused(opn(n_sel=3), selection)
    refused(opn(sel_=np.ascontiguousarray([1, 2], dtype=np.int32)), selection)
    refused(opn(sel_=np.ascontiguousarray([1, 1], dtype=np.int32)), selection)
    refused(opn(mb=0), fn + ": max_block_sample_frames must be >= 1")
    refused(opn(n=0), fn + ": frame_len must be in [1, 67108864]")
    refused(opn(s=0), fn + ": stride must be >= 1")
    refused(opn(mb=(1 << 40) + 1), fn + ": max_block_sample_frames or stride too large")
    refused(opn(s=1, mb=1 << 31), fn + ": too many frames for one launch")
    refused(opn(s=1, mb=1 << 30), fn + ": too many frames for one launch")           # the call over both planes, not a plane, is too long

    ld = ah._width(vb, pkg, "tracked_ext")
    ld += ld & 1
    bs = [Bufs(vb, pkg, ld), Bufs(vb, pkg, ld)]
    dev = vb.to_device(np.zeros(64, np.int16))
    blk = np.ascontiguousarray(audio[FIRST:FIRST + NEXT])

    def entries(rec=lambda k: bs[k].rec.ptr, st=lambda k: bs[k].st.ptr, po=lambda k: bs[k].po):
        ent, keep = (pkg.ChannelOutputs * 2)(), []
        for k in range(2):
            ent[k].records, ent[k].status3 = rec(k), st(k)
            o = po(k)
            keep.append(o)
            if o is not None:
                ent[k].outputs = C.pointer(o)
        return ent, keep

    def paths(path=lambda k: bs[k].path.ptr, commit=lambda k: bs[k].commit.ptr):
        ent = (pkg.ChannelPathOutputs * 2)()
        for k in range(2):
            ent[k].out_path, ent[k].d_commit = path(k), commit(k)
        return ent
    with vb.session_channels(p, ext, track, channels=2, select=sel, frame_len=N, stride=H, max_block=MB) as sess, \
            vb.session_channels(p, ext, None, channels=2, select=sel, frame_len=N, stride=H, max_block=MB) as untracked, \
            vb.session(p, ext, track, frame_len=N, stride=H, max_block=MB) as single:

        def bind(s=sess.handle, peak_ref=1.0, pending=64, ent=paths(), ld_=2):
            return L.vbx_session_path_bind_channels(s, peak_ref, pending, ent, ld_)
        fn = "vbx_session_path_bind_channels"
        refused(bind(s=None), fn + ": null session", ctx=False)
        refused(bind(s=single.handle), fn + ": the session was opened with vbx_session_open: bind with vbx_session_path_bind")
        refused(bind(s=untracked.handle), fn + ": the session was opened without h_track: it has no candidate lists")
        refused(bind(ent=None), fn + ": null outputs")
        refused(bind(ent=paths(path=lambda k: None if k == 1 else bs[k].path.ptr)), fn + ": null out_path or d_commit")
        refused(bind(ent=paths(commit=lambda k: None if k == 1 else bs[k].commit.ptr)), fn + ": null out_path or d_commit")
        refused(bind(ld_=1), fn + ": path_ld must be >= 2")
        refused(bind(pending=0), fn + ": max_pending must be in [1, 2^24]")
        refused(bind(peak_ref=float("nan")), fn + ": silence_threshold > 0 needs a finite peak_ref >= 0")
        assert bind() == 0
        refused(bind(pending=65), fn + ": a bound session keeps its peak_ref and max_pending (vbx_session_reset drops the binding)")
        refused(bind(peak_ref=2.0), fn + ": a bound session keeps its peak_ref and max_pending (vbx_session_reset drops the binding)")
        sess.reset()                                                         # the binding goes: the pushes below are those of `fresh`
        first = sess.push(audio[:FIRST])
        refused(bind(), fn + ": bind before the first push or after vbx_session_reset")
        before = sess.info()
        good, keep = entries()

        def push(fn_=L.vbx_session_push_channels, s=sess.handle, block=blk.ctypes.data, n=NEXT, ent=good, rld=ld, sld=8):
            return fn_(s, block, n, ent, rld, sld, None)
        for fn_, fn, device in ((L.vbx_session_push_channels, "vbx_session_push_channels", False),
                                (L.vbx_session_push_channels_device, "vbx_session_push_channels_device", True)):
            full = dict(fn_=fn_, block=dev.ptr) if device else dict(fn_=fn_)
            refused(push(fn_=fn_, s=None), fn + ": null session", ctx=False)
            refused(push(fn_=fn_, s=single.handle), fn + ": the session was opened with vbx_session_open: push with vbx_session_push")
            refused(push(fn_=fn_, block=None), fn + ": null block")
            refused(push(fn_=fn_, n=MB + 1), fn + ": the block is larger than the session's max_block_sample_frames")
            refused(push(ent=None, **full), fn + ": null outputs")
            refused(push(rld=ld + 1, **full), fn + ": record_ld must be even and >= vbx_record_doubles(params)")
            refused(push(rld=ld - 2, **full), fn + ": record_ld must be even and >= vbx_record_doubles(params)")
            refused(push(ent=entries(rec=lambda k: None if k == 1 else bs[k].rec.ptr)[0], **full), fn + ": null argument")
            refused(push(sld=3, **full), fn + ": status_ld must be >= the frames the push delivers")
            refused(push(ent=entries(rec=lambda k: bs[k].rec.ptr + 8 * k)[0], **full), fn + ": records must be 16-byte aligned")
            refused(push(ent=entries(rec=lambda k: bs[0].rec.ptr)[0], **full), fn + ": the channels' records overlap")
            refused(push(ent=entries(rec=lambda k: bs[0].rec.ptr + k * 3 * ld * 8)[0], **full), fn + ": the channels' records overlap")
            one = lambda o: (lambda k: o if k == 1 else bs[k].po)
            refused(push(ent=entries(po=one(None))[0], **full), fn + ": the tracked form needs outputs->cand and ->count")
            for o, text in ((bs[1].lists(pkg, cand=False), ": the tracked form needs outputs->cand and ->count"),
                            (bs[1].lists(pkg, count=False), ": the tracked form needs outputs->cand and ->count"),
                            (bs[1].lists(pkg, peak=False), ": a silence_threshold needs outputs->peak"),
                            (bs[1].lists(pkg, index=True), ": outputs->index must be NULL: the caller runs the path (vbx_pitch_path_f64)")):
                ent, keep2 = entries(po=one(o))
                refused(push(ent=ent, **full), fn + text)
        refused(push(fn_=L.vbx_session_push_channels_device, block=dev.ptr + 1, n=8), "vbx_session_push_channels_device: the block needs its type's alignment")
        for fn_, fn in ((L.vbx_session_push, "vbx_session_push"), (L.vbx_session_push_device, "vbx_session_push_device")):
            refused(fn_(sess.handle, blk.ctypes.data, NEXT, bs[0].rec.ptr, ld, bs[0].st.ptr, 8, C.byref(bs[0].po), None),
                    fn + ": the session was opened with vbx_session_open_channels: push with vbx_session_push_channels")
        assert sess.info() == before and untracked.info() == (0, 0, 0) and single.info() == (0, 0, 0)
        second = sess.push(blk)
    with vb.session_channels(p, ext, track, channels=2, select=sel, frame_len=N, stride=H, max_block=MB) as fresh:
        want = fresh.push(audio[:FIRST]), fresh.push(blk)
    for k in range(2):
        assert first[k][0].shape[0] == 4 and second[k][0].shape[0] == 4
        assert _bits(first[k]) == _bits(want[0][k]) and _bits(second[k]) == _bits(want[1][k])
    dev.free()
    for b in bs:
        b.free()


def test_pool_refusal_texts(vb, pkg, pcm):
    L, refused = vb.L, Refusals(vb)
    p = ah._params(pkg)
    ext, track = ah._form(pkg, "tracked_ext")
    h = C.c_void_p()

    def opn(ctx=vb.ctx, hf=None, no_fmt=False, n=N, s=H, prm=p, e=ext, t=track, ms=3, mb=MB, mt=3 * MB, out=h, no_params=False):
        f = _fmt(pkg, **(hf or {}))
        rc = L.vbx_pool_open(ctx, None if no_fmt else C.byref(f), n, s, None if no_params else C.byref(prm), None if e is None else C.byref(e),
                             None if t is None else C.byref(t), ms, mb, mt, None if out is None else C.byref(out))
        assert not h.value
        return rc
    fn = "vbx_pool_open"
    refused(opn(ctx=None), fn + ": null context", ctx=False)
    _open_texts(refused, opn, fn, pkg)
    for bad in (dict(channels=2), dict(channels=0), dict(channels=2, channel=1)):
        refused(opn(hf=bad), fn + ": a pool's streams are mono: channels must be 1 and channel 0")
    refused(opn(ms=0), fn + ": max_streams must be >= 1")
    refused(opn(mb=0), fn + ": need 1 <= max_block_sample_frames <= max_tick_sample_frames")
    refused(opn(mt=MB - 1), fn + ": need 1 <= max_block_sample_frames <= max_tick_sample_frames")
    refused(opn(n=0), fn + ": frame_len must be in [1, VBX_MAX_FRAME_LEN]: longer frames take one vbx_session per stream")
    refused(opn(n=4097, s=2048), fn + ": frame_len must be in [1, VBX_MAX_FRAME_LEN]: longer frames take one vbx_session per stream")
    refused(opn(s=0), fn + ": stride must be in [1, 2^40]")
    refused(opn(s=(1 << 40) + 1), fn + ": stride must be in [1, 2^40]")
    refused(opn(ms=1 << 31), fn + ": max_streams or max_tick_sample_frames too large")
    refused(opn(mt=(1 << 40) + 1), fn + ": max_streams or max_tick_sample_frames too large")
    refused(opn(ms=1 << 26, mt=1 << 40), fn + ": too many frames for one launch")

    ld = ah._width(vb, pkg, "tracked_ext")
    ld += ld & 1
    b = Bufs(vb, pkg, ld)
    dev = vb.to_device(np.zeros(64, np.int16))
    blk = np.ascontiguousarray(pcm[FIRST:FIRST + NEXT])
    big = np.zeros(MB + 1, np.int16)
    E = pkg.PoolEntry
    with vb.pool(p, ext, track, format=1, frame_len=N, stride=H, max_streams=3, max_block=MB, max_tick=MB + H) as pool:
        first = pool.push([(1, pcm[:FIRST])])
        before = [pool.info(k) for k in range(3)]

        def push(fn_=L.vbx_pool_push, q=pool.handle, ents=(E(1, blk.ctypes.data, NEXT),), no_ents=False, rec=b.rec.ptr, rld=ld, st=b.st.ptr, sld=8, po=b.po):
            arr = (E * max(len(ents), 1))(*ents)
            return fn_(q, None if no_ents else arr, len(ents), rec, rld, st, sld, None if po is None else C.byref(po), None, None)
        for fn_, fn, device in ((L.vbx_pool_push, "vbx_pool_push", False), (L.vbx_pool_push_device, "vbx_pool_push_device", True)):
            full = dict(fn_=fn_, ents=(E(1, dev.ptr, NEXT),)) if device else dict(fn_=fn_)
            src = dev.ptr if device else blk.ctypes.data
            refused(push(fn_=fn_, q=None), fn + ": null pool", ctx=False)
            refused(push(fn_=fn_, no_ents=True), fn + ": null entries")
            refused(push(fn_=fn_, ents=(E(3, src, NEXT),)), fn + ": a stream outside [0, max_streams)")
            refused(push(fn_=fn_, ents=(E(-1, src, NEXT),)), fn + ": a stream outside [0, max_streams)")
            refused(push(fn_=fn_, ents=(E(1, src, NEXT), E(1, src, H))), fn + ": a stream is listed twice in one tick")
            refused(push(fn_=fn_, ents=(E(1, None, NEXT),)), fn + ": null block")
            refused(push(fn_=fn_, ents=(E(1, big.ctypes.data, big.size),)), fn + ": a block is larger than the pool's max_block_sample_frames")
            refused(push(fn_=fn_, ents=(E(0, src, MB), E(1, src, NEXT))), fn + ": the tick's blocks are larger than the pool's max_tick_sample_frames")
            refused(push(rec=None, **full), fn + ": null argument")
            refused(push(rec=b.rec.ptr + 8, **full), fn + ": records must be 16-byte aligned")
            refused(push(rld=ld + 1, **full), fn + ": record_ld must be even and >= vbx_record_doubles(params)")
            refused(push(rld=ld - 2, **full), fn + ": record_ld must be even and >= vbx_record_doubles(params)")
            refused(push(sld=3, **full), fn + ": status_ld must be >= the rows the tick delivers")
            refused(push(po=None, **full), fn + ": the tracked form needs h_outputs->cand and ->count")
            refused(push(po=b.lists(pkg, cand=False), **full), fn + ": the tracked form needs h_outputs->cand and ->count")
            refused(push(po=b.lists(pkg, count=False), **full), fn + ": the tracked form needs h_outputs->cand and ->count")
            refused(push(po=b.lists(pkg, peak=False), **full), fn + ": a silence_threshold needs h_outputs->peak")
            refused(push(po=b.lists(pkg, index=True), **full), fn + ": h_outputs->index must be NULL: the caller runs the path (vbx_pitch_path_f64)")
        refused(push(fn_=L.vbx_pool_push_device, ents=(E(1, dev.ptr + 1, NEXT),)), "vbx_pool_push_device: a block needs its type's alignment")
        refused(L.vbx_pool_mark_utterance(pool.handle, 3), "vbx_pool_mark_utterance: a stream outside [0, max_streams)")
        refused(L.vbx_pool_reset_stream(pool.handle, -1), "vbx_pool_reset_stream: a stream outside [0, max_streams)")
        refused(L.vbx_pool_info(pool.handle, 3, None, None, None), "vbx_pool_info: a stream outside [0, max_streams)")
        assert [pool.info(k) for k in range(3)] == before
        second = pool.push([(1, blk)])
    with vb.pool(p, ext, track, format=1, frame_len=N, stride=H, max_streams=3, max_block=MB, max_tick=MB + H) as fresh:
        want = fresh.push([(1, pcm[:FIRST])]), fresh.push([(1, blk)])
    assert first[1].shape[0] == 4 and second[1].shape[0] == 4
    assert _bits(first) == _bits(want[0]) and _bits(second) == _bits(want[1])
    dev.free()
    b.free()
