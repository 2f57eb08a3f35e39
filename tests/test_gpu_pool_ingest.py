"""The ingest kernel of a session pool's tick (k_pool.hip, pool_ingest_<fmt>) on its own, through vbx_internal_pool_ingest, on a real
MI355X.  An entry is a slot's old tail (elements of the plane's type), a block in the pool's sample format, a plane region and a new
tail; a position p < 0 is element old_len + p of the old tail, p >= 0 sample p of the block.  The kernel must write, per call, ONE
plane -- entry after entry its region [first, first + span), the next region ceil(span / stride) hops behind, zeros in the gap of
fewer than `stride` elements between them -- and every entry's new tail [carry_first, carry_first + carry_len) into that entry's carry
destination.  Every comparison is BIT FOR BIT against numpy on integer views (NaN payloads, the sign of zero and subnormals count;
24- / 32-bit / unsigned 8-bit PCM are the correctly rounded quotients, G.711 the ITU tables of tests/sample8_cases.py) and covers the
whole plane and the whole tail.  All eight formats; 1, 2 and 40 entries; old tails of 0, 1, G - 1, G, G + 1 elements and the full
bound VBX_SHARD_WARM_FRAMES * stride + frame_len - 1; blocks of 0, 1, 7, 8, 9, 15, 16, 17 and 4099 samples; every source residue
within 16 bytes the format allows; entries that complete no frame (the tail alone is written); entries whose region begins inside the
block (stride > frame_len: the samples between are dropped).  Planes and tails sit in a fenced arena (tests/layout_arena.py), now and
then off a 16-byte boundary: nothing outside them is written, and the old tails -- the slot's other carry buffer -- are inputs of
the arena, so they are checked to be untouched.  Poison sits directly behind every block and around every old tail."""
import ctypes as C
import itertools

import numpy as np
import pytest

import layout_arena as la
import sample8_cases as s8
from test_gpu_clips_pack import _poison
from test_gpu_session_ingest import _specials
from test_gpu_unpack import F32, F64, OUT, PCM16, PCM24, PCM32, _bits, _expected, _source

pytestmark = pytest.mark.gpu

FORMATS = (PCM16, PCM24, PCM32, F32, F64) + s8.FORMATS8
OUT_T = {**OUT, **s8.OUT}
SRC_BYTES = {PCM16: 2, PCM24: 3, PCM32: 4, F32: 4, F64: 8, s8.U8: 1, s8.ULAW: 1, s8.ALAW: 1}
ALIGN = {PCM16: 2, PCM24: 1, PCM32: 4, F32: 4, F64: 8, s8.U8: 1, s8.ULAW: 1, s8.ALAW: 1}
N, H = 400, 160
BOUND = 64 * H + N - 1
BLOCKS = (0, 1, 7, 8, 9, 15, 16, 17, 4099)


def _block_source(fmt, rng, n):
    """n samples of the format: (what each becomes in the plane, their bytes)"""
    if fmt in s8.FORMATS8:
        codes = s8.random_codes(rng, n)
        return s8.decode(fmt, codes).astype(OUT_T[fmt]), codes
    vals, raw = _source(fmt, rng, n)
    if fmt in (F32, F64) and n >= 6:
        vals = _specials(fmt, vals)
        raw = vals.view(np.uint8).copy()
    return _expected(fmt, vals).astype(OUT_T[fmt]), raw


def _tail_source(fmt, rng, n):
    """n elements of the plane's type, as an earlier ingest wrote them"""
    if fmt in s8.FORMATS8:
        return s8.decode(fmt, rng.integers(0, 256, n).astype(np.uint8)).astype(OUT_T[fmt])
    vals, _ = _source(fmt, rng, n)
    v = _expected(fmt, vals).astype(OUT_T[fmt])
    return _specials(fmt, v) if fmt in (F32, F64) and n >= 6 else v


class _Image:
    """one byte image: items at chosen residues of their address modulo 16, poison between them"""

    def __init__(self, fmt):
        self.fmt, self.parts, self.size = fmt, [], 0

    def add(self, raw, residue):
        pad = 16 + (residue - (self.size + 16)) % 16
        self.parts.append(_poison(self.fmt, pad))
        self.size += pad
        off = self.size
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        self.parts += [raw, _poison(self.fmt, 32)]
        self.size += raw.size + 32
        return off

    def bytes(self):
        """(the arena takes elements of 2, 4 or 8 bytes: the image goes in as 16-bit words)"""
        img = np.concatenate(self.parts + [np.zeros(16 + (-self.size) % 16, np.uint8)])
        return img.view(np.uint16)


def _entries(fmt, rng):
    """the calls of one format: lists of entries (old_len, n_new, first, span, carry_first, carry_len, residue)"""
    G = 16 // np.dtype(OUT_T[fmt]).itemsize
    tails = (0, 1, G - 1, G, G + 1, BOUND)
    residues = list(range(0, 16, ALIGN[fmt]))
    k = itertools.count()

    def entry(L, n, kind, residue):
        seq = L + n
        if kind == "frames":                                    # the region is everything at hand; the tail keeps a part of it
            first, span = -L, seq
        elif kind == "none":                                    # no frame completes: the tail alone
            first, span = 0, 0
        elif kind == "inside":                                  # the region begins inside the block, the samples before it are dropped
            first, span = (3, n - 5) if n >= 6 else (-L, seq)
        else:                                                   # a region that ends before the block does
            first, span = (-L, seq - 2) if seq > 2 else (-L, seq)
        keep = (0, 1, G + 1, seq, seq // 2)[next(k) % 5]
        keep = min(keep, seq)
        return (L, n, first, span, n - keep, keep, residue)

    kinds = ("frames", "none", "inside", "short")
    calls = []
    for i, (L, n) in enumerate(itertools.product(tails, BLOCKS)):                # one entry: every tail with every block
        calls.append([entry(L, n, kinds[i % 4], residues[i % len(residues)])])
    for r in residues:                                                           # every source residue, wide loads and ragged ends
        calls.append([entry(G + 1, 4099, "frames", r)])
        calls.append([entry(0, 17, "frames", r)])
    for i, ((La, na), (Lb, nb)) in enumerate(itertools.product(itertools.product((0, G - 1, BOUND), (1, 9, 16, 4099)), repeat=2)):
        if i % 3 == 0:                                                           # two entries
            calls.append([entry(La, na, kinds[i % 4], residues[i % len(residues)]), entry(Lb, nb, kinds[(i // 4) % 4], residues[(5 * i + 1) % len(residues)])])
    for order in (0, 1):                                                         # forty entries, entries without frames first, inside and last
        es = []
        for j in range(40):
            L, n = tails[(j + order) % len(tails)], BLOCKS[(j * (5 if order else 1) + order) % len(BLOCKS)]
            kind = "none" if (order and j in (0, 1, 20, 39)) else kinds[(j + order) % 4]
            es.append(entry(L, n, kind, residues[(j + order) % len(residues)]))
        calls.append(es)
    return calls


@pytest.mark.parametrize("fmt", FORMATS, ids=[f"fmt{f}" for f in FORMATS])
def test_pool_ingest_against_numpy(vb, pkg, fmt):
    rng = np.random.default_rng(9100 + fmt)
    out_t = OUT_T[fmt]
    es = np.dtype(out_t).itemsize
    calls = _entries(fmt, rng)
    assert {len(c) for c in calls} == {1, 2, 40}
    blocks, tails_img = _Image(fmt), _Image(fmt)
    plan = []                                                                    # per call: [(entry, block offset, tail offset, seq values)]
    tail_res = la.RESIDUES[es]
    for ci, call in enumerate(calls):
        rows = []
        for ei, e in enumerate(call):
            L, n = e[0], e[1]
            new_vals, raw = _block_source(fmt, rng, n)
            old_vals = _tail_source(fmt, rng, L)
            b_off = blocks.add(raw, e[6])
            t_off = tails_img.add(old_vals, tail_res[(ci + ei) % len(tail_res)] if (ci + ei) % 3 == 2 else 0)
            rows.append((e, b_off, t_off, np.concatenate([old_vals, new_vals]).astype(out_t)))
        plan.append(rows)
    ar = la.Arena(la.DeviceBackend(vb), f"pool_ingest fmt {fmt}")
    ar.input("blocks", blocks.bytes())
    ar.input("tails", tails_img.bytes())
    totals = []
    for ci, rows in enumerate(plan):
        off = total = 0
        for e, _, _, _ in rows:
            if e[3]:
                total = off + e[3]
                off += -(-e[3] // H) * H
        totals.append(total)
        if total:                                                                # now and then a plane off a 16-byte boundary
            ar.output(f"p{ci}", out_t, 1, total, residue=tail_res[ci % len(tail_res)] if ci % 4 == 3 else 0)
        for ei, (e, _, _, _) in enumerate(rows):
            if e[5]:
                ar.output(f"c{ci}_{ei}", out_t, 1, e[5], residue=tail_res[(ci + ei) % len(tail_res)] if (ci + ei) % 5 == 4 else 0)
    ar.place()

    def run(ci, fmt_=fmt, stride=H, shift=0, bad_first=False, null_plane=False):
        rows = plan[ci]
        h = (pkg.voxbox._PoolIngestEntry * len(rows))()
        for ei, (e, b_off, t_off, _) in enumerate(rows):
            L, n, first, span, cf, cl, _ = e
            h[ei].d_block = ar["blocks"] + b_off + shift if n else None
            h[ei].n_new = n
            h[ei].d_old = ar["tails"] + t_off if L else None
            h[ei].old_len = L
            h[ei].d_carry = ar[f"c{ci}_{ei}"] if cl else None
            h[ei].first, h[ei].span = (first - 1 if bad_first and ei == 0 else first), span
            h[ei].carry_first, h[ei].carry_len = cf, cl
        total = C.c_size_t(12345)
        plane = ar[f"p{ci}"] if totals[ci] and not null_plane else None
        return vb.L.vbx_internal_pool_ingest(vb.ctx, fmt_, h, len(rows), stride, plane, C.byref(total)), int(total.value)

    # rejected calls write nothing (the canaries of that call's planes and tails are checked with everything else)
    big = next(ci for ci, rows in enumerate(plan) if len(rows) == 1 and rows[0][0][3] > 1000 and rows[0][0][2] < 0)
    assert run(big, fmt_=0)[0] == -1 and run(big, stride=0)[0] == -1 and run(big, null_plane=True)[0] == -1
    assert run(big, bad_first=True)[0] == -1                                     # a region that would read before the old tail
    if ALIGN[fmt] > 1:
        assert run(big, shift=1)[0] == -1                                        # a block off its type's alignment
    for ci in range(len(plan)):
        rc, got_total = run(ci)
        vb._check(rc)
        assert got_total == totals[ci], (ci, got_total, totals[ci])
    out = ar.finish()                                # the fences around every plane and tail, and the inputs (the old tails) untouched
    seen = dict(gap=False, none=False, inside=False)
    for ci, rows in enumerate(plan):
        want = np.zeros(totals[ci], out_t)
        off = 0
        for ei, (e, _, _, seq) in enumerate(rows):
            L, n, first, span, cf, cl, _ = e
            if span:
                want[off:off + span] = seq[L + first:L + first + span]
                nxt = off + -(-span // H) * H
                seen["gap"] |= nxt > off + span and ei + 1 < len(rows) and any(r[0][3] for r in rows[ei + 1:])
                seen["inside"] |= first > 0
                off = nxt
            else:
                seen["none"] = True
            if cl:
                got = out[f"c{ci}_{ei}"][0]
                w = seq[L + cf:L + cf + cl]
                bad = np.nonzero(_bits(got) != _bits(w))[0]
                assert bad.size == 0, (fmt, "call", ci, "entry", ei, e, "tail: first differing element", int(bad[0]), bad.size)
        if totals[ci]:
            got = out[f"p{ci}"][0]
            bad = np.nonzero(_bits(got) != _bits(want))[0]
            assert bad.size == 0, (fmt, "call", ci, [r[0] for r in rows][:4], "plane: first differing element", int(bad[0]), bad.size,
                                   got[bad[0]], want[bad[0]])
    assert all(seen.values()), seen
