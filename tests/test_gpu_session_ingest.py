"""The ingest kernel of a live session (k_session.hip, session_ingest_<fmt>) on its own, through vbx_internal_session_ingest, on a
real MI355X: out[0, keep) = old[drop, drop + keep), out[keep, keep + n_new) = the selected channel of the new block as the type the
frame loop reads.  Every comparison is BIT FOR BIT against numpy (integer views: NaN payloads, the sign of zero and subnormals
count); 24- and 32-bit PCM are the correctly rounded quotients, as in tests/test_gpu_unpack.py, whose recordings these are.  Every
output sits inside a fenced arena (tests/layout_arena.py): the canaries on both sides must be intact."""
import itertools

import numpy as np
import pytest

import layout_arena as la
from test_gpu_unpack import F32, F64, OUT, PCM16, PCM24, PCM32, _bits, _expected, _source

pytestmark = pytest.mark.gpu

KEEPS = (0, 1, 7, 8, 31_919)
DROPS = (0, 1, 3, 480)
NEWS = (0, 1, 15, 16, 17, 480, 5_000)
SRC_BYTES = {PCM16: 2, PCM24: 3, PCM32: 4, F32: 4, F64: 8}
# (format, channels, byte offset of the raw source): every format at 1, 2 and 3 channels from an aligned source, a PCM24 source at an
# odd byte address and a PCM16 source at an odd element
CASES = [(f, c, 0) for f in (PCM16, PCM24, PCM32, F32, F64) for c in (1, 2, 3)] + [(PCM24, 1, 1), (PCM24, 2, 1), (PCM16, 1, 2), (PCM16, 2, 2)]


def _specials(fmt, v):
    """a NaN with a payload, -0.0 and a subnormal among the first samples of a float array (bit patterns the copy must keep)"""
    if fmt == F32:
        v[:6] = np.array([0x7FC12345, 0x80000000, 0x00000001, 0xFFA00001, 0x807FFFFF, 0x7F800001], np.uint32).view(np.float32)
    elif fmt == F64:
        v[:6] = np.array([0x7FF8000000012345, 0x8000000000000000, 0x0000000000000001, 0xFFF4000000000001, 0x800FFFFFFFFFFFFF,
                          0x7FF0000000000001], np.uint64).view(np.float64)
    return v


@pytest.mark.parametrize("fmt,channels,src_off", CASES, ids=[f"fmt{f}-{c}ch-off{o}" for f, c, o in CASES])
def test_ingest_against_numpy(vb, fmt, channels, src_off):
    rng = np.random.default_rng(100 * fmt + 10 * channels + src_off)
    channel = channels - 1
    # the old carry: values of the OUTPUT type (what an earlier ingest wrote)
    ov, _ = _source(fmt, rng, max(DROPS) + max(KEEPS) + 8)
    old = _specials(fmt, _expected(fmt, ov).astype(OUT[fmt]))
    old[-3:] = old[:3]
    vals, raw = _source(fmt, rng, max(NEWS) * channels)
    if fmt in (F32, F64):
        sel = vals.reshape(-1, channels)
        sel[:6, channel] = _specials(fmt, np.zeros(6, vals.dtype))
        raw = vals.view(np.uint8).copy()
    d_old = vb.to_device(old)
    d_raw = vb.to_device(np.concatenate([np.zeros(src_off, np.uint8), raw]), np.uint8)
    combos = [c for c in itertools.product(KEEPS, DROPS, NEWS) if c[0] + c[2] > 0]
    ar = la.Arena(la.DeviceBackend(vb), f"session_ingest fmt {fmt} channels {channels} offset {src_off}")
    for i, (keep, drop, n_new) in enumerate(combos):
        # (a destination off a 16-byte boundary now and then: the element form, the same bits)
        ar.output(f"o{i}", OUT[fmt], 1, keep + n_new, residue=8 if i % 7 == 3 else 0)
    ar.place()
    for i, (keep, drop, n_new) in enumerate(combos):
        vb._check(vb.L.vbx_internal_session_ingest(vb.ctx, fmt, channels, channel, d_old.ptr, drop, keep, d_raw.ptr + src_off, n_new, ar[f"o{i}"]))
    # nothing to write: no launch, no pointer needed
    assert vb.L.vbx_internal_session_ingest(vb.ctx, fmt, channels, channel, None, 0, 0, None, 0, None) == 0
    out = ar.finish()                                                            # (the fences are checked here)
    d_old.free(); d_raw.free()
    picked = _expected(fmt, vals.reshape(-1, channels)[:, channel]).astype(OUT[fmt])
    for i, (keep, drop, n_new) in enumerate(combos):
        want = np.concatenate([old[drop:drop + keep], picked[:n_new]])
        got = out[f"o{i}"][0]
        bad = np.nonzero(_bits(got) != _bits(want))[0]
        assert bad.size == 0, (fmt, channels, src_off, "keep/drop/n_new", keep, drop, n_new, "first differing element", int(bad[0]), bad.size)


def test_ingest_rejections(vb):
    L, c = vb.L, vb.ctx
    buf = vb.empty(64, np.float64)
    assert L.vbx_internal_session_ingest(None, PCM16, 1, 0, buf.ptr, 0, 1, buf.ptr, 1, buf.ptr) == -1
    for fmt, ch, sel in ((0, 1, 0), (6, 1, 0), (PCM16, 0, 0), (PCM16, 2, 2), (PCM16, 1, -1)):
        assert L.vbx_internal_session_ingest(c, fmt, ch, sel, buf.ptr, 0, 1, buf.ptr, 1, buf.ptr + 256) == -1, (fmt, ch, sel)
    assert L.vbx_internal_session_ingest(c, F64, 1, 0, buf.ptr, 0, 1, buf.ptr, 1, None) == -1                # no destination
    assert L.vbx_internal_session_ingest(c, F64, 1, 0, None, 0, 1, buf.ptr, 1, buf.ptr + 256) == -1          # a tail to keep, no old carry
    assert L.vbx_internal_session_ingest(c, F64, 1, 0, buf.ptr, 0, 1, None, 1, buf.ptr + 256) == -1          # new samples, no block
    assert L.vbx_internal_session_ingest(c, F32, 1, 0, buf.ptr, 0, 1, buf.ptr + 2, 1, buf.ptr + 256) == -1   # a float source off its alignment
    assert L.vbx_internal_session_ingest(c, F64, 1, 0, buf.ptr, 0, 1, buf.ptr, 1, buf.ptr + 4) == -1         # a double carry off its alignment
    vb.sync()
    buf.free()
