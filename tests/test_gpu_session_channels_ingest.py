"""The ingest kernel of a multi-channel live session (k_session_channels.hip, session_ingest_all_<fmt>) on its own, through
vbx_internal_session_ingest_channels, on a real MI355X: plane p of the output = the old plane p from element `drop`, `keep` elements,
then channel sel[p] of the new block as the type the frame loop reads.  Every comparison is BIT FOR BIT against numpy (integer views:
NaN payloads, the sign of zero and subnormals count); 24- and 32-bit PCM are the correctly rounded quotients, as in
tests/test_gpu_unpack.py, whose recordings these are.  Every output sits inside a fenced arena (tests/layout_arena.py) with one
plane more than the call selects: the canaries around the planes, behind each plane's keep + n_new elements and in the spare plane
must be intact."""
import itertools

import numpy as np
import pytest

import layout_arena as la
from test_gpu_session_ingest import _specials
from test_gpu_unpack import F32, F64, OUT, PCM16, PCM24, PCM32, _bits, _expected, _source

pytestmark = pytest.mark.gpu

SRC_BYTES = {PCM16: 2, PCM24: 3, PCM32: 4, F32: 4, F64: 8}
GROUP = {PCM16: 8, PCM24: 2, PCM32: 2, F32: 4, F64: 2}             # elements in a lane's 16 output bytes
TILE_BYTES = 8192
# (channels, selection): mono; stereo reversed; one of three (odd sample-frame widths: 9 bytes at 24 bits); a subset of five; all 64
SELECTIONS = [(1, [0]), (2, [1, 0]), (3, [2]), (5, [4, 0, 2]), (64, list(range(64)))]
# every format and selection from an aligned source; a PCM24 source at an odd byte address and a PCM16 source at an odd element; and
# sample frames too wide for a tile (more than 512 bytes: 70 doubles, 200 packed 24-bit samples), which no tile can serve
CASES = [(f, c, s, 0) for f in (PCM16, PCM24, PCM32, F32, F64) for c, s in SELECTIONS] + \
        [(PCM24, 1, [0], 1), (PCM24, 5, [4, 0, 2], 1), (PCM16, 1, [0], 2), (PCM16, 5, [4, 0, 2], 2)] + \
        [(F64, 70, [69, 0, 33], 0), (F64, 70, list(range(3, 67)), 0), (PCM24, 200, [199, 1], 0)]


def _tile(fmt, channels):
    """sample frames per LDS tile (0: the sample frames are too wide for sixteen of them to fit)"""
    fb = channels * SRC_BYTES[fmt]
    return (TILE_BYTES // fb) & ~15 if fb <= TILE_BYTES // 16 else 0


def test_the_cases_reach_every_path():
    """(the test's own arithmetic, no GPU work: the cases hold tiled shapes, the narrowest tile and shapes no tile can serve)"""
    tiles = [_tile(f, c) for f, c, _, _ in CASES]
    assert all(t == 0 or t >= 16 for t in tiles) and tiles.count(0) == 3 and 16 in tiles
    assert _tile(F64, 64) == 16 and _tile(PCM16, 1) == 4096 and _tile(PCM24, 3) == 896
    assert _tile(F64, 65) == 0 and _tile(F64, 70) == 0 and _tile(PCM24, 200) == 0


@pytest.mark.parametrize("fmt,channels,sel,src_off", CASES, ids=[f"fmt{f}-{c}ch-sel{len(s)}-off{o}" for f, c, s, o in CASES])
def test_ingest_all_against_numpy(vb, fmt, channels, sel, src_off):
    rng = np.random.default_rng(1000 * fmt + 10 * channels + src_off)
    G, K = GROUP[fmt], len(sel)
    T = _tile(fmt, channels) or 48                                      # (no tile: the same sizes around a stand-in of 48 sample frames)
    keeps = (0, 1, G - 1, G, G + 1)
    news = (1, T - 1, T, T + 1, 3 * T + G + 1)                          # a few tiles and a ragged end
    drop, old_ld = 3, max(keeps) + 11
    # the old carry: K planes of the OUTPUT type (what an earlier ingest wrote)
    ov, _ = _source(fmt, rng, K * old_ld)
    old = _expected(fmt, ov).astype(OUT[fmt]).reshape(K, old_ld)
    old[0] = _specials(fmt, old[0])
    vals, raw = _source(fmt, rng, max(news) * channels)
    if fmt in (F32, F64):
        vals.reshape(-1, channels)[:6, sel[0]] = _specials(fmt, np.zeros(6, vals.dtype))
        raw = vals.view(np.uint8).copy()
    d_old = vb.to_device(old.reshape(-1))
    d_raw = vb.to_device(np.concatenate([np.zeros(src_off, np.uint8), raw]), np.uint8)
    h_sel = np.ascontiguousarray(sel, dtype=np.int32)
    combos = list(itertools.product(keeps, news))
    ar = la.Arena(la.DeviceBackend(vb), f"session_ingest_all fmt {fmt} channels {channels} selection {sel} offset {src_off}")
    lds = []
    for i, (keep, n_new) in enumerate(combos):
        # plane pitches that keep every plane on a 16-byte boundary -- and now and then one that does not, or a destination off one
        # (the per-element stores, the same bits); one plane more than the call selects
        ld = (keep + n_new + 7) // 8 * 8 + 8 + (1 if i % 6 == 4 else 0)
        lds.append(ld)
        ar.output(f"o{i}", OUT[fmt], K + 1, keep + n_new, ld=ld, residue=8 if i % 11 == 7 else 0)
    ar.place()

    def call(i, keep, n_new, **kw):
        a = dict(fmt=fmt, channels=channels, sel=h_sel.ctypes.data, n_sel=K, old=d_old.ptr, old_ld=old_ld, drop=drop, keep=keep,
                 raw=d_raw.ptr + src_off, n_new=n_new, out=ar[f"o{i}"], out_ld=lds[i])
        a.update(kw)
        return vb.L.vbx_internal_session_ingest_channels(vb.ctx, a["fmt"], a["channels"], a["sel"], a["n_sel"], a["old"], a["old_ld"], a["drop"],
                                                         a["keep"], a["raw"], a["n_new"], a["out"], a["out_ld"])
    # rejected calls write nothing (the fences and the planes' canaries are checked with everything else)
    assert call(0, *combos[0], sel=None) == -1 and call(0, *combos[0], n_sel=0) == -1 and call(0, *combos[0], n_sel=channels + 1) == -1
    assert call(0, *combos[0], fmt=0) == -1 and call(0, *combos[0], out=None) == -1 and call(0, *combos[0], raw=None) == -1
    assert call(0, *combos[0], out_ld=combos[0][0] + combos[0][1] - 1) == -1          # a plane that does not fit its pitch
    assert call(0, max(keeps), 1, old_ld=drop + max(keeps) - 1) == -1
    if K > 1:
        twice = np.ascontiguousarray([sel[0]] * K, dtype=np.int32)
        assert call(0, *combos[0], sel=twice.ctypes.data) == -1                         # a repeated channel
    assert call(0, 0, 0, old=None, raw=None, out=None) == 0                             # nothing to write: no launch, no pointer needed
    for i, (keep, n_new) in enumerate(combos):
        vb._check(call(i, keep, n_new))
    out = ar.finish()                                                            # (the fences and the padding behind each plane are checked here)
    d_old.free(); d_raw.free()
    picked = [_expected(fmt, vals.reshape(-1, channels)[:, c]).astype(OUT[fmt]) for c in sel]
    for i, (keep, n_new) in enumerate(combos):
        got = out[f"o{i}"]
        assert la.unwritten(got[K:]).shape[0] == got[K:].size, ("the plane behind the selection was written", keep, n_new)
        for p in range(K):
            want = np.concatenate([old[p, drop:drop + keep], picked[p][:n_new]])
            bad = np.nonzero(_bits(got[p]) != _bits(want))[0]
            assert bad.size == 0, (fmt, channels, sel, src_off, "keep/n_new/plane", keep, n_new, p, "first differing element", int(bad[0]), bad.size)
