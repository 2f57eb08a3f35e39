"""The pack kernel of vbx_analyze_clips (k_clips.hip, clips_pack_<fmt>) on its own, through vbx_internal_clips_pack, on a real
MI355X: the clips of one group gathered into one plane of the type the frame loop reads -- clip b + 1 starts ceil(len_b / stride)
hops behind clip b, zeros in the gap of fewer than `stride` elements between them.  Every comparison is BIT FOR BIT against numpy
(integer views: NaN payloads, the sign of zero and subnormals count; 24- and 32-bit PCM are the correctly rounded quotients, as in
tests/test_gpu_unpack.py) and covers the WHOLE plane: samples, then zeros in each gap.  All five formats, every source pointer residue
within 16 bytes the format allows, an even and an odd stride, lengths 0, 1, stride - 1, stride, stride + 1 and a few thousand, and 1, 2
and 40 clips in a group.  Every plane sits inside a fenced arena (tests/layout_arena.py), now and then off a 16-byte boundary (the
element-wise stores); poison -- NaN for the float formats, 0x7f bytes for PCM -- sits directly behind every source clip, where an
over-read would carry it into a gap that must hold zeros."""
import ctypes as C
import itertools

import numpy as np
import pytest

import layout_arena as la
from test_gpu_session_ingest import _specials
from test_gpu_unpack import F32, F64, OUT, PCM16, PCM24, PCM32, _bits, _expected, _source

pytestmark = pytest.mark.gpu

SRC_BYTES = {PCM16: 2, PCM24: 3, PCM32: 4, F32: 4, F64: 8}
ALIGN = {PCM16: 2, PCM24: 1, PCM32: 4, F32: 4, F64: 8}             # what a clip pointer must be a multiple of
STRIDES = (480, 37)
CASES = [(f, s) for f in (PCM16, PCM24, PCM32, F32, F64) for s in STRIDES]


def _poison(fmt, nbytes):
    if fmt == F32:
        return np.full(nbytes // 4 + 1, np.nan, np.float32).view(np.uint8)[:nbytes]
    if fmt == F64:
        return np.full(nbytes // 8 + 1, np.nan, np.float64).view(np.uint8)[:nbytes]
    return np.full(nbytes, 0x7F, np.uint8)


class _Sources:
    """one byte image of every clip of a test: each at a chosen residue of its address modulo 16, poison directly behind it (and
    in the padding before it)"""

    def __init__(self, fmt, rng):
        self.fmt, self.rng, self.parts, self.size, self.clips = fmt, rng, [], 0, []

    def add(self, length, residue):
        fmt = self.fmt
        pad = 16 + (residue - (self.size + 16)) % 16                            # (for F32 / F64 the padding keeps the element grid: whole NaNs)
        self.parts.append(_poison(fmt, pad))
        self.size += pad
        vals, raw = _source(fmt, self.rng, length)
        if fmt in (F32, F64) and length >= 6:
            vals = _specials(fmt, vals)
            raw = vals.view(np.uint8).copy()
        off = self.size
        self.parts += [raw, _poison(fmt, 32)]
        self.size += raw.size + 32
        self.clips.append((off, length, _expected(fmt, vals).astype(OUT[fmt])))
        return len(self.clips) - 1

    def upload(self, vb):
        self.dev = vb.to_device(np.concatenate(self.parts), np.uint8)
        assert self.dev.ptr % 16 == 0
        return self.dev


def _layout(lengths, stride):
    offs, off, total = [], 0, 0
    for ln in lengths:
        offs.append(off)
        total = off + ln
        off += -(-ln // stride) * stride
    return offs, total


@pytest.mark.parametrize("fmt,stride", CASES, ids=[f"fmt{f}-stride{s}" for f, s in CASES])
def test_pack_against_numpy(vb, fmt, stride):
    rng = np.random.default_rng(7000 + 10 * fmt + stride)
    residues = list(range(0, 16, ALIGN[fmt]))
    lens = [0, 1, stride - 1, stride, stride + 1, 3000 + stride // 2]
    src = _Sources(fmt, rng)
    calls = []                                                                  # lists of clip ids
    # one clip: every residue at every length
    for r, ln in itertools.product(residues, lens):
        calls.append([src.add(ln, r)])
    # two clips: every pair of lengths, the residues rotating
    for i, (a, b) in enumerate(itertools.product(lens, lens)):
        calls.append([src.add(a, residues[i % len(residues)]), src.add(b, residues[(3 * i + 1) % len(residues)])])
    # forty clips: every length several times in two orders, the residues rotating; zero-length clips first, inside and last
    for order in (0, 1):
        ls = [lens[(k * (5 if order else 1) + order) % len(lens)] for k in range(40)]
        ls[0], ls[-1] = (0, 0) if order else (ls[0], ls[-1])
        calls.append([src.add(ln, residues[(k + order) % len(residues)]) for k, ln in enumerate(ls)])
    d_src = src.upload(vb)
    es = np.dtype(OUT[fmt]).itemsize
    out_res = la.RESIDUES[es]
    ar = la.Arena(la.DeviceBackend(vb), f"clips_pack fmt {fmt} stride {stride}")
    plans = []
    for i, ids in enumerate(calls):
        lengths = [src.clips[c][1] for c in ids]
        offs, total = _layout(lengths, stride)
        plans.append((lengths, offs, total))
        if total:                                                               # now and then a plane off a 16-byte boundary
            ar.output(f"o{i}", OUT[fmt], 1, total, residue=out_res[i % len(out_res)] if i % 4 == 3 else 0)
    ar.place()

    def call(ids, out, fmt_=fmt, stride_=stride, null_clip=False, shift=0):
        n = len(ids)
        h_clip = (C.c_void_p * n)(*[None if null_clip else d_src.ptr + src.clips[c][0] + shift for c in ids])
        h_len = (C.c_size_t * n)(*[src.clips[c][1] for c in ids])
        total = C.c_size_t(12345)
        return vb.L.vbx_internal_clips_pack(vb.ctx, fmt_, h_clip, h_len, n, stride_, out, C.byref(total)), int(total.value)

    # rejected calls write nothing (the canaries of plane 0's arena entry are checked with everything else)
    big = next(i for i, p in enumerate(plans) if p[2] > 1000)
    assert call(calls[big], ar[f"o{big}"], fmt_=0)[0] == -1 and call(calls[big], ar[f"o{big}"], stride_=0)[0] == -1
    assert call(calls[big], ar[f"o{big}"], null_clip=True)[0] == -1 and call(calls[big], None)[0] == -1
    if ALIGN[fmt] > 1:
        assert call(calls[big], ar[f"o{big}"], shift=1)[0] == -1                 # a clip off its type's alignment
    for i, ids in enumerate(calls):
        lengths, offs, total = plans[i]
        rc, got_total = call(ids, ar[f"o{i}"] if total else None)
        vb._check(rc)
        assert got_total == total, (i, got_total, total)
    out = ar.finish()                                                            # (the fences around every plane are checked here)
    d_src.free()
    for i, ids in enumerate(calls):
        lengths, offs, total = plans[i]
        if not total:
            continue
        want = np.zeros(total, OUT[fmt])
        for c, off in zip(ids, offs):
            want[off:off + src.clips[c][1]] = src.clips[c][2]
        got = out[f"o{i}"][0]
        bad = np.nonzero(_bits(got) != _bits(want))[0]
        assert bad.size == 0, (fmt, stride, "call", i, "lengths", lengths[:6], "first differing element", int(bad[0]), bad.size,
                               got[bad[0]], want[bad[0]])
