"""vbx_unpack_samples and vbx_unpack_channels on the 8-bit formats (VBX_SAMPLE_U8 / ULAW / ALAW) on a real MI355X.  Every comparison
is BIT FOR BIT against numpy (uint64 / uint16 views): unsigned 8-bit PCM is numpy.float64(b - 128) / 127, G.711 the ITU tables restated
in tests/sample8_cases.py.  One source image per format holds every case's bytes at its own residue of the address modulo 16, with
0x7f bytes around each; every output sits in ONE fenced arena (tests/layout_arena.py), on and off a 16-byte boundary, with canaries
behind element n and between the planes.  Sizes: nothing, one, around a lane's 16 output bytes (7, 8, 9 and 15, 16, 17) and 4099,
which is behind the last whole LDS tile of every channel count with a tail left over."""
import numpy as np
import pytest

import layout_arena as la
import sample8_cases as s8
from sample8_cases import ALAW, FORMATS8, GROUP, OUT, TAG, U8, ULAW

pytestmark = pytest.mark.gpu

E_INVALID = -1
SIZES = (0, 1, 7, 8, 9, 15, 16, 17, 4099)
RESIDUES = tuple(range(16))
OUT_RES = {U8: (0, 8), ULAW: (0, 2, 8, 14), ALAW: (0, 6, 8, 10)}       # destinations on and off a 16-byte boundary


class _Image:
    """the sources of one test in one device buffer: each at a chosen residue modulo 16, 0x7f bytes before and behind it"""

    def __init__(self):
        self.parts, self.size = [], 0

    def add(self, raw, residue):
        pad = 16 + (residue - (self.size + 16)) % 16
        self.parts += [np.full(pad, 0x7F, np.uint8), raw, np.full(16, 0x7F, np.uint8)]
        off = self.size + pad
        self.size = off + raw.size + 16
        return off

    def upload(self, vb):
        self.dev = vb.to_device(np.concatenate(self.parts), np.uint8)
        assert self.dev.ptr % 16 == 0
        return self.dev


def _selections(channels):
    if channels == 1:
        return [[0]]
    singles = [[c] for c in (range(channels) if channels <= 3 else (0, 3, channels - 1))]      # every single channel (of eight: three)
    sels = singles + [list(range(channels))]
    if channels >= 3:
        sels.append([channels - 1, 1, 0] if channels == 3 else [6, 4, 1])                     # a subset in reverse order
    return sels


def test_every_code(vb):
    """all 256 codes of each format, in order, through both the wide and the element path"""
    codes = np.arange(256, dtype=np.uint8)
    for fmt in FORMATS8:
        for off in (0, 1):
            src = vb.to_device(np.concatenate([np.zeros(off, np.uint8), codes]), np.uint8)
            out = vb.empty(256, OUT[fmt])
            vb._check(vb.L.vbx_unpack_samples(vb.ctx, src.ptr + off, 256, fmt, 1, 0, out.ptr))
            got = out.numpy()
            src.free(); out.free()
            assert got.dtype == OUT[fmt] and np.array_equal(s8.bits(got), s8.bits(s8.decode(fmt, codes))), (fmt, off)
    g = s8.decode(ULAW, codes)
    assert g[0x7f] == 0 and g[0xff] == 0 and g[0] == -32124 and s8.decode(ALAW, codes)[0xaa] == 32256


@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_unpack_samples_against_numpy(vb, fmt):
    rng = np.random.default_rng(800 + fmt)
    img, cases = _Image(), []
    for channels in (1, 2, 3, 8):
        for n in SIZES:
            for r in (RESIDUES if channels <= 2 else (0, 1, 4, 7, 8, 13)):
                codes = s8.random_codes(rng, max(n, 1) * channels)
                off = img.add(codes, r)
                for channel in (range(channels) if channels <= 3 else (0, 5, 7)):
                    cases.append((channels, channel, n, off, codes))
    d = img.upload(vb)
    ar = la.Arena(la.DeviceBackend(vb), f"unpack_{TAG[fmt]}")
    for i, (channels, channel, n, off, codes) in enumerate(cases):
        ar.output(f"o{i}", OUT[fmt], 1, max(n, 4) + 3, residue=OUT_RES[fmt][i % len(OUT_RES[fmt])] if i % 3 == 1 else 0)
    ar.place()
    for i, (channels, channel, n, off, codes) in enumerate(cases):
        vb._check(vb.L.vbx_unpack_samples(vb.ctx, d.ptr + off, n, fmt, channels, channel, ar[f"o{i}"]))
    out = ar.finish()                                                            # every fence byte intact: no overrun
    d.free()
    for i, (channels, channel, n, off, codes) in enumerate(cases):
        got = out[f"o{i}"][0]
        want = s8.decode(fmt, codes.reshape(-1, channels)[:n, channel])
        bad = np.nonzero(s8.bits(got[:n]) != s8.bits(want))[0]
        assert bad.size == 0, (TAG[fmt], "channels/channel/n/source residue", channels, channel, n, (d.ptr + off) % 16, "first", int(bad[0]), bad.size)
        assert la.unwritten(got[n:]).shape[0] == got.size - n, (TAG[fmt], channels, channel, n, "written past element n")


@pytest.mark.parametrize("fmt", FORMATS8, ids=[TAG[f] for f in FORMATS8])
def test_unpack_channels_against_numpy(vb, fmt):
    rng = np.random.default_rng(900 + fmt)
    G = GROUP[fmt]
    img, cases = _Image(), []
    for channels in (1, 2, 3, 8):
        for n in SIZES:
            for r in RESIDUES:
                codes = s8.random_codes(rng, max(n, 1) * channels)
                off = img.add(codes, r)
                for k, sel in enumerate(_selections(channels)):
                    if n < 4099 and r not in (0, 1, 4, 8) and k:                # (the small sizes: every residue for the first selection)
                        continue
                    # a pitch that keeps the planes' lane groups aligned (the tiled form where a tile fits), and one that does not
                    for ld in ((n + 127) // 128 * 128 + 128, (n + G) // G * G + 1):
                        cases.append((channels, sel, n, off, codes, ld))
    d = img.upload(vb)
    ar = la.Arena(la.DeviceBackend(vb), f"unpack_all_{TAG[fmt]}")
    for i, (channels, sel, n, off, codes, ld) in enumerate(cases):
        ar.output(f"o{i}", OUT[fmt], len(sel) + 1, max(n, 1), ld=ld, residue=OUT_RES[fmt][i % len(OUT_RES[fmt])] if i % 5 == 2 else 0)
    ar.place()
    for i, (channels, sel, n, off, codes, ld) in enumerate(cases):
        h_sel = np.ascontiguousarray(sel, dtype=np.int32)
        vb._check(vb.L.vbx_unpack_channels(vb.ctx, d.ptr + off, n, fmt, channels, h_sel.ctypes.data, len(sel), ar[f"o{i}"], ld))
    out = ar.finish()                                                            # (the fences and the padding between planes are checked here)
    d.free()
    assert any(n >= s8.tile_frames(c) for c, _, n, *_ in cases if c > 1) and s8.tile_frames(2) == 4096 and s8.tile_frames(3) == 2720
    for i, (channels, sel, n, off, codes, ld) in enumerate(cases):
        got = out[f"o{i}"]
        assert la.unwritten(got[len(sel):]).shape[0] == got[len(sel):].size, ("the plane behind the selection was written", channels, sel, n)
        for p, c in enumerate(sel):
            want = s8.decode(fmt, codes.reshape(-1, channels)[:n, c])
            bad = np.nonzero(s8.bits(got[p, :n]) != s8.bits(want))[0]
            assert bad.size == 0, (TAG[fmt], "channels/selection/n/ld/source residue/plane", channels, sel, n, ld, (d.ptr + off) % 16, p,
                                   "first", int(bad[0]), bad.size)
            assert la.unwritten(got[p, n:]).shape[0] == got.shape[1] - n, (TAG[fmt], channels, sel, n, "written past element n")


def test_errors(vb):
    src, out = vb.to_device(np.zeros(256, np.uint8), np.uint8), vb.empty(64)
    fn, fa = vb.L.vbx_unpack_samples, vb.L.vbx_unpack_channels
    one = np.zeros(1, np.int32)
    for bad in (0, 6, 7, 15, 19, -1, 255):
        assert fn(vb.ctx, src.ptr, 8, bad, 1, 0, out.ptr) == E_INVALID, bad
        assert fa(vb.ctx, src.ptr, 8, bad, 1, one.ctypes.data, 1, out.ptr, 8) == E_INVALID, bad
    for fmt in FORMATS8:
        assert fn(vb.ctx, src.ptr, 8, fmt, 2, 2, out.ptr) == E_INVALID and fn(vb.ctx, src.ptr, 8, fmt, 0, 0, out.ptr) == E_INVALID
        assert fn(vb.ctx, src.ptr, 8, fmt, 2, -1, out.ptr) == E_INVALID
        assert fn(vb.ctx, None, 8, fmt, 1, 0, out.ptr) == E_INVALID and fn(vb.ctx, src.ptr, 8, fmt, 1, 0, None) == E_INVALID
        assert fn(vb.ctx, src.ptr + 3, 8, fmt, 1, 0, out.ptr) == 0            # an 8-bit source has no alignment requirement
        assert fn(vb.ctx, None, 0, fmt, 1, 0, None) == 0                      # nothing to do
        two = np.array([1, 1], np.int32)
        assert fa(vb.ctx, src.ptr, 8, fmt, 2, two.ctypes.data, 2, out.ptr, 8) == E_INVALID      # a repeated channel
        assert fa(vb.ctx, src.ptr, 8, fmt, 2, None, 1, out.ptr, 8) == E_INVALID and fa(vb.ctx, src.ptr, 8, fmt, 2, two.ctypes.data, 3, out.ptr, 8) == E_INVALID
        assert fa(vb.ctx, src.ptr, 8, fmt, 1, one.ctypes.data, 1, out.ptr, 7) == E_INVALID      # plane_ld < n
    assert fn(vb.ctx, src.ptr, 8, U8, 1, 0, out.ptr + 4) == E_INVALID         # a double destination at 4 mod 8
    assert fn(vb.ctx, src.ptr, 8, ULAW, 1, 0, out.ptr + 1) == E_INVALID and fn(vb.ctx, src.ptr, 8, ALAW, 1, 0, out.ptr + 1) == E_INVALID
    assert fn(vb.ctx, src.ptr, 8, ULAW, 1, 0, out.ptr) == 0                   # the context is usable afterwards
    assert np.array_equal(out.numpy().view(np.int16)[:8], np.full(8, s8.TABLE[ULAW][0]))
    src.free(); out.free()


def test_every_launch_is_profiled(vb):
    rng = np.random.default_rng(5)
    sel = np.array([1, 0], np.int32)
    vb.profile(True)
    vb.profile_reset()
    try:
        for fmt in FORMATS8:
            src = vb.to_device(s8.random_codes(rng, 1000), np.uint8)
            out = vb.empty(1024, OUT[fmt])
            vb._check(vb.L.vbx_unpack_samples(vb.ctx, src.ptr, 500, fmt, 2, 1, out.ptr))
            vb._check(vb.L.vbx_unpack_channels(vb.ctx, src.ptr, 500, fmt, 2, sel.ctypes.data, 2, out.ptr, 512))
            vb.sync()
            src.free(); out.free()
        rep = vb.profile_report()
    finally:
        vb.profile(False)
    for fmt in FORMATS8:
        for name in ("unpack_" + TAG[fmt], "unpack_all_" + TAG[fmt]):
            assert name in rep and rep[name][1] == 1, (name, sorted(rep))
    assert not any(k.startswith("unpack") and k.endswith(("pcm16", "f64")) for k in rep), sorted(rep)      # no second pass in another format
