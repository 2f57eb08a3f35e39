"""The 8-bit instantiations of the kernels that build the frame loop's plane, each on its own on a real MI355X: the ingest of a live
session (session_ingest_<fmt>, vbx_internal_session_ingest), of a multi-channel session (session_ingest_all_<fmt>,
vbx_internal_session_ingest_channels) and the pack kernel of vbx_analyze_clips (clips_pack_<fmt>, vbx_internal_clips_pack), for
VBX_SAMPLE_U8 / ULAW / ALAW.  The cases are those of tests/test_gpu_session_ingest.py, tests/test_gpu_session_channels_ingest.py and
tests/test_gpu_clips_pack.py around a 160-sample hop: blocks of 1, stride - 1, stride and a few thousand sample frames behind a
carried tail (kept decoded, in the plane's type), sources at odd byte addresses, clips of length 0, 1, stride - 1, stride + 1 and a
few thousand, 1, 2 and 40 clips.  The WHOLE plane is compared with numpy, bit for bit (tests/sample8_cases.py); every output sits in
a fenced arena (tests/layout_arena.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import layout_arena as la
import sample8_cases as s8
from sample8_cases import FORMATS8, GROUP, OUT, TAG

pytestmark = pytest.mark.gpu

STRIDE = 160
NEWS = (1, STRIDE - 1, STRIDE, 5000)
OFFSETS = (0, 1, 3, 8)                                  # byte offsets of the raw block: on a 16-byte boundary, odd, on 8


@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_session_ingest_against_numpy(vb, fmt):
    rng = np.random.default_rng(300 + fmt)
    G = GROUP[fmt]
    keeps, drops = (0, 1, G - 1, G, G + 1, 241), (0, 3)
    old = s8.decode(fmt, s8.random_codes(rng, max(drops) + max(keeps) + 8)).astype(OUT[fmt])
    d_old = vb.to_device(old)
    for channels in (1, 2, 3):
        channel = channels - 1
        codes = s8.random_codes(rng, max(NEWS) * channels)
        picked = s8.decode(fmt, codes.reshape(-1, channels)[:, channel])
        d_raw = vb.to_device(np.concatenate([np.full(16, 0x7F, np.uint8), codes, np.full(16, 0x7F, np.uint8)]), np.uint8)
        combos = list(itertools.product(keeps, drops, NEWS, OFFSETS))
        ar = la.Arena(la.DeviceBackend(vb), f"session_ingest_{TAG[fmt]} channels {channels}")
        for i, (keep, drop, n_new, off) in enumerate(combos):
            ar.output(f"o{i}", OUT[fmt], 1, keep + n_new, residue=8 if i % 7 == 3 else 0)
        ar.place()
        for i, (keep, drop, n_new, off) in enumerate(combos):
            # (a block that starts `off` BYTES into the source: sample frames from byte `off` on, so the expected samples shift with it)
            vb._check(vb.L.vbx_internal_session_ingest(vb.ctx, fmt, channels, channel, d_old.ptr, drop, keep, d_raw.ptr + 16 + off * channels,
                                                       min(n_new, max(NEWS) - off), ar[f"o{i}"]))
        out = ar.finish()
        d_raw.free()
        for i, (keep, drop, n_new, off) in enumerate(combos):
            m = min(n_new, max(NEWS) - off)
            want = np.concatenate([old[drop:drop + keep], picked[off:off + m]])
            got = out[f"o{i}"][0]
            bad = np.nonzero(s8.bits(got[:keep + m]) != s8.bits(want))[0]
            assert bad.size == 0, (TAG[fmt], "channels/keep/drop/n_new/offset", channels, keep, drop, n_new, off, "first", int(bad[0]), bad.size)
            assert la.unwritten(got[keep + m:]).shape[0] == got.size - keep - m
    for bad_fmt in (0, 6, 7, 15, 19):
        assert vb.L.vbx_internal_session_ingest(vb.ctx, bad_fmt, 1, 0, d_old.ptr, 0, 1, d_old.ptr, 1, d_old.ptr + 256) == -1, bad_fmt
    assert vb.L.vbx_internal_session_ingest(vb.ctx, fmt, 1, 0, d_old.ptr, 0, 1, d_old.ptr, 1, d_old.ptr + (4 if fmt == s8.U8 else 1)) == -1
    vb.sync()
    d_old.free()


# (channels, selection): mono; stereo reversed; one of three; a subset of five; all 64
SELECTIONS = [(1, [0]), (2, [1, 0]), (3, [2]), (5, [4, 0, 2]), (64, list(range(64)))]
CASES_ALL = [(f, c, s) for f in FORMATS8 for c, s in SELECTIONS]


@pytest.mark.parametrize("fmt,channels,sel", CASES_ALL, ids=[f"{TAG[f]}-{c}ch-sel{len(s)}" for f, c, s in CASES_ALL])
def test_session_ingest_all_against_numpy(vb, fmt, channels, sel):
    rng = np.random.default_rng(1000 * fmt + channels)
    G, K = GROUP[fmt], len(sel)
    T = s8.tile_frames(channels)
    assert T >= 16
    keeps = (0, 1, G - 1, G, G + 1)
    news = (1, STRIDE - 1, STRIDE, T - 1, T, T + 1, 2 * T + G + 1)          # a few tiles and a ragged end
    drop, old_ld = 3, max(keeps) + 11
    old = s8.decode(fmt, s8.random_codes(rng, K * old_ld)).astype(OUT[fmt]).reshape(K, old_ld)
    codes = s8.random_codes(rng, (max(news) + max(OFFSETS)) * channels)
    d_old = vb.to_device(old.reshape(-1))
    d_raw = vb.to_device(np.concatenate([np.full(16, 0x7F, np.uint8), codes, np.full(16, 0x7F, np.uint8)]), np.uint8)
    h_sel = np.ascontiguousarray(sel, dtype=np.int32)
    combos = [(k, n, OFFSETS[(i + j) % len(OFFSETS)]) for i, k in enumerate(keeps) for j, n in enumerate(news)] + \
             [(G, 2 * T + G + 1, o) for o in OFFSETS] + [(1, T, o) for o in OFFSETS]
    ar = la.Arena(la.DeviceBackend(vb), f"session_ingest_all_{TAG[fmt]} channels {channels} selection {sel}")
    lds = []
    for i, (keep, n_new, off) in enumerate(combos):
        ld = (keep + n_new + 7) // 8 * 8 + 8 + (1 if i % 6 == 4 else 0)
        lds.append(ld)
        ar.output(f"o{i}", OUT[fmt], K + 1, keep + n_new, ld=ld, residue=8 if i % 11 == 7 else 0)
    ar.place()
    for i, (keep, n_new, off) in enumerate(combos):
        vb._check(vb.L.vbx_internal_session_ingest_channels(vb.ctx, fmt, channels, h_sel.ctypes.data, K, d_old.ptr, old_ld, drop, keep,
                                                            d_raw.ptr + 16 + off * channels, n_new, ar[f"o{i}"], lds[i]))
    for bad_fmt in (0, 6, 7, 15, 19):
        assert vb.L.vbx_internal_session_ingest_channels(vb.ctx, bad_fmt, channels, h_sel.ctypes.data, K, d_old.ptr, old_ld, drop, 1,
                                                         d_raw.ptr, 1, ar["o0"], lds[0]) == -1, bad_fmt
    out = ar.finish()                                                            # (the fences and the padding behind each plane are checked here)
    d_old.free(); d_raw.free()
    frames = codes.reshape(-1, channels)
    for i, (keep, n_new, off) in enumerate(combos):
        got = out[f"o{i}"]
        assert la.unwritten(got[K:]).shape[0] == got[K:].size, ("the plane behind the selection was written", keep, n_new)
        for p, c in enumerate(sel):
            want = np.concatenate([old[p, drop:drop + keep], s8.decode(fmt, frames[off:off + n_new, c])])
            bad = np.nonzero(s8.bits(got[p]) != s8.bits(want))[0]
            assert bad.size == 0, (TAG[fmt], channels, sel, "keep/n_new/offset/plane", keep, n_new, off, p, "first", int(bad[0]), bad.size)


def _layout(lengths, stride):
    offs, off, total = [], 0, 0
    for ln in lengths:
        offs.append(off)
        total = off + ln
        off += -(-ln // stride) * stride
    return offs, total


CASES_PACK = [(f, s) for f in FORMATS8 for s in (STRIDE, 37)]


@pytest.mark.parametrize("fmt,stride", CASES_PACK, ids=[f"{TAG[f]}-stride{s}" for f, s in CASES_PACK])
def test_clips_pack_against_numpy(vb, fmt, stride):
    rng = np.random.default_rng(7000 + 10 * fmt + stride)
    lens = [0, 1, stride - 1, stride, stride + 1, 3000 + stride // 2]
    parts, size, clips = [], 0, []                                              # one byte image of every clip, 0x7f bytes around each

    def add(length, residue):
        nonlocal size
        pad = 16 + (residue - (size + 16)) % 16
        codes = s8.random_codes(rng, length)
        parts.extend([np.full(pad, 0x7F, np.uint8), codes, np.full(32, 0x7F, np.uint8)])
        clips.append((size + pad, length, s8.decode(fmt, codes).astype(OUT[fmt])))
        size += pad + length + 32
        return len(clips) - 1
    calls = []
    for r, ln in itertools.product(range(16), lens):                             # one clip: every residue at every length
        calls.append([add(ln, r)])
    for i, (a, b) in enumerate(itertools.product(lens, lens)):                   # two clips: every pair of lengths
        calls.append([add(a, i % 16), add(b, (3 * i + 1) % 16)])
    for order in (0, 1):                                                         # forty clips, zero-length ones first, inside and last
        ls = [lens[(k * (5 if order else 1) + order) % len(lens)] for k in range(40)]
        ls[0], ls[-1] = (0, 0) if order else (ls[0], ls[-1])
        calls.append([add(ln, (k + order) % 16) for k, ln in enumerate(ls)])
    d_src = vb.to_device(np.concatenate(parts), np.uint8)
    assert d_src.ptr % 16 == 0
    out_res = la.RESIDUES[np.dtype(OUT[fmt]).itemsize]
    ar = la.Arena(la.DeviceBackend(vb), f"clips_pack_{TAG[fmt]} stride {stride}")
    plans = []
    for i, ids in enumerate(calls):
        offs, total = _layout([clips[c][1] for c in ids], stride)
        plans.append((offs, total))
        if total:
            ar.output(f"o{i}", OUT[fmt], 1, total, residue=out_res[i % len(out_res)] if i % 4 == 3 else 0)
    ar.place()

    def call(ids, out, fmt_=fmt, null_clip=False):
        n = len(ids)
        h_clip = (C.c_void_p * n)(*[None if null_clip else d_src.ptr + clips[c][0] for c in ids])
        h_len = (C.c_size_t * n)(*[clips[c][1] for c in ids])
        total = C.c_size_t(12345)
        return vb.L.vbx_internal_clips_pack(vb.ctx, fmt_, h_clip, h_len, n, stride, out, C.byref(total)), int(total.value)
    big = next(i for i, p in enumerate(plans) if p[1] > 1000)
    for bad_fmt in (0, 6, 7, 15, 19):
        assert call(calls[big], ar[f"o{big}"], fmt_=bad_fmt)[0] == -1, bad_fmt
    assert call(calls[big], ar[f"o{big}"], null_clip=True)[0] == -1 and call(calls[big], None)[0] == -1
    for i, ids in enumerate(calls):
        rc, got_total = call(ids, ar[f"o{i}"] if plans[i][1] else None)
        vb._check(rc)
        assert got_total == plans[i][1], (i, got_total, plans[i][1])
    out = ar.finish()
    d_src.free()
    for i, ids in enumerate(calls):
        offs, total = plans[i]
        if not total:
            continue
        want = np.zeros(total, OUT[fmt])
        for c, off in zip(ids, offs):
            want[off:off + clips[c][1]] = clips[c][2]
        got = out[f"o{i}"][0]
        bad = np.nonzero(s8.bits(got) != s8.bits(want))[0]
        assert bad.size == 0, (TAG[fmt], stride, "call", i, "lengths", [clips[c][1] for c in ids][:6], "first", int(bad[0]), bad.size)
