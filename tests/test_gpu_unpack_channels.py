"""vbx_unpack_channels on a real MI355X: every selected channel of interleaved sample frames in one pass, each plane BIT FOR BIT what
vbx_unpack_samples writes for that channel and what numpy gives (uint16 / uint32 / uint64 views, so NaN payloads, the sign of zero and
subnormals count): numpy.float64(s) / 8388607 and / 2147483647 for 24- and 32-bit PCM, the raw bits for the rest.  The planes sit in
fenced arenas (tests/layout_arena.py) as the rows of one output whose leading dimension is plane_ld: the padding between planes and
the fences around them must keep their canaries.  Sizes lie around a lane's 16 output bytes (7, 8, 9), around the tiles of the
wider sample frames (511, 512, 513) and, at 4099, behind several tiles of every shape with a tail left over."""
import numpy as np
import pytest

import layout_arena as la

pytestmark = pytest.mark.gpu

E_INVALID = -1
PCM16, PCM24, PCM32, F32, F64 = 1, 2, 3, 4, 5
FORMATS = [PCM16, PCM24, PCM32, F32, F64]
NAMES = {PCM16: "unpack_all_pcm16", PCM24: "unpack_all_pcm24", PCM32: "unpack_all_pcm32", F32: "unpack_all_f32", F64: "unpack_all_f64"}
OUT = {PCM16: np.int16, PCM24: np.float64, PCM32: np.float64, F32: np.float32, F64: np.float64}
SRC_BYTES = {PCM16: 2, PCM24: 3, PCM32: 4, F32: 4, F64: 8}
SIZES = (0, 1, 7, 8, 9, 511, 512, 513, 4099)


def _pack24(s):
    return np.ascontiguousarray(np.ascontiguousarray(s, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)


def _source(fmt, rng, total):
    """`total` samples of the format: (what each becomes, as the output type; the bytes the library reads).  Floats are random BIT
    patterns -- NaNs with payloads, infinities, subnormals among them -- with -0.0, the smallest subnormals and signalling NaNs put in."""
    if fmt == PCM16:
        v = rng.integers(-32768, 32768, total).astype(np.int16)
        return v, v.view(np.uint8).copy()
    if fmt == PCM24:
        v = rng.integers(-(1 << 23), 1 << 23, total).astype(np.int32)
        v[:3] = (-(1 << 23), (1 << 23) - 1, 0)[:min(3, total)]
        return v.astype(np.float64) / np.float64(8388607.0), _pack24(v)
    if fmt == PCM32:
        v = rng.integers(-(1 << 31), 1 << 31, total).astype(np.int32)
        v[:3] = (-(1 << 31), (1 << 31) - 1, -1)[:min(3, total)]
        return v.astype(np.float64) / np.float64(2147483647.0), v.view(np.uint8).copy()
    if fmt == F32:
        w = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
        special = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0x7F800001, 0xFFBFFFFF], dtype=np.uint32)
        w[:min(special.size, total)] = special[:total]
        return w.view(np.float32), w.view(np.uint8).copy()
    w = rng.integers(0, 1 << 63, total, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, total, dtype=np.uint64)
    special = np.array([0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF8C0DEC0DE0001, 0x7FF0000000000001,
                        0xFFF7FFFFFFFFFFFF], dtype=np.uint64)
    w[:min(special.size, total)] = special[:total]
    return w.view(np.float64), w.view(np.uint8).copy()


def _selections(channels):
    sels = [list(range(channels)), list(range(channels))[::-1], [channels // 2], [channels - 1, 0]]
    out = []
    for s in sels:
        if len(set(s)) == len(s) and s not in out:
            out.append(s)
    return out


def _planes(vb, fmt, src_addr, n, channels, sel, ld, residue=0, label=""):
    """the call into a fenced [n_sel, n] output with leading dimension ld: the planes (canaries and fences checked)"""
    a = la.Arena(la.DeviceBackend(vb), label)
    a.output("planes", OUT[fmt], len(sel), n, ld=ld, residue=residue)
    a.place()
    s = np.array(sel, dtype=np.int32)
    vb._check(vb.L.vbx_unpack_channels(vb.ctx, src_addr, n, fmt, channels, s.ctypes.data, s.size, a["planes"], ld))
    return a.finish()["planes"]


def _one_channel(vb, fmt, src_addr, n, channels, channel):
    """vbx_unpack_samples on that channel"""
    out = vb.empty(max(n, 1), OUT[fmt])
    vb._check(vb.L.vbx_unpack_samples(vb.ctx, src_addr, n, fmt, channels, channel, out.ptr))
    got = out.numpy()[:n]
    out.free()
    return got


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_plane_is_the_single_channel_call(vb, fmt, channels):
    rng = np.random.default_rng(1000 * fmt + channels)
    for n in SIZES:
        want, raw = _source(fmt, rng, max(n, 1) * channels)
        want = want.reshape(-1, channels)[:n]
        src = vb.to_device(np.concatenate([raw, np.zeros(16, np.uint8)]), np.uint8)
        single = [_one_channel(vb, fmt, src.ptr, n, channels, c) for c in range(channels)]
        for c in range(channels):
            la.assert_same_bits(f"{NAMES[fmt]} channels {channels} n {n}", f"unpack_samples channel {c} against numpy", single[c],
                                np.ascontiguousarray(want[:, c]))
        for sel in _selections(channels):
            for ld in (n, (n + 7) // 8 * 8 + 32):
                label = f"{NAMES[fmt]} channels {channels} n {n} selection {sel} plane_ld {ld}"
                planes = _planes(vb, fmt, src.ptr, n, channels, sel, ld, label=label)
                assert planes.shape == (len(sel), n), label
                for k, c in enumerate(sel):
                    la.assert_same_bits(label, f"plane {k} against unpack_samples", planes[k], single[c])
        src.free()


@pytest.mark.parametrize("fmt", FORMATS)
def test_sources_and_destinations_off_the_wide_boundaries(vb, fmt):
    """A source one element in (PCM24: one, two and three bytes in) and a destination at 8 mod 16: the bits are the same."""
    rng = np.random.default_rng(77 + fmt)
    channels, n = 3, 4099
    want, raw = _source(fmt, rng, n * channels)
    want = want.reshape(-1, channels)
    offsets = (1, 2, 3) if fmt == PCM24 else (SRC_BYTES[fmt],)
    cases = [(off, 0) for off in offsets] + [(0, 8), (offsets[0], 8)]
    for src_off, residue in cases:
        src = vb.to_device(np.concatenate([np.zeros(src_off, np.uint8), raw, np.zeros(16, np.uint8)]), np.uint8)
        for sel, ld in (([0, 1, 2], n + 5), ([2, 0], n)):
            label = f"{NAMES[fmt]} source +{src_off} B, destination at {residue} mod 16, selection {sel}, plane_ld {ld}"
            planes = _planes(vb, fmt, src.ptr + src_off, n, channels, sel, ld, residue=residue, label=label)
            for k, c in enumerate(sel):
                la.assert_same_bits(label, f"plane {k}", planes[k], np.ascontiguousarray(want[:, c]))
        src.free()


def test_sixty_four_of_sixty_five_channels(vb):
    rng = np.random.default_rng(65)
    channels, n = 65, 100
    want, raw = _source(PCM16, rng, n * channels)
    want = want.reshape(-1, channels)
    src = vb.to_device(raw, np.uint8)
    sel = list(range(64, 0, -1))                                # 64 channels, reversed, channel 0 left out
    planes = _planes(vb, PCM16, src.ptr, n, channels, sel, 128, label="64 of 65")
    for k, c in enumerate(sel):
        la.assert_same_bits("64 of 65", f"plane {k}", planes[k], np.ascontiguousarray(want[:, c]))
    # 65 of 65 is over the cap: refused, nothing written
    a = la.Arena(la.DeviceBackend(vb), "65 of 65")
    a.output("planes", np.int16, 65, n, ld=128)
    a.place()
    s = np.arange(65, dtype=np.int32)
    assert vb.L.vbx_unpack_channels(vb.ctx, src.ptr, n, PCM16, channels, s.ctypes.data, 65, a["planes"], 128) == E_INVALID
    out = a.finish()["planes"]
    assert la.unwritten(out).shape[0] == out.size
    src.free()


@pytest.mark.parametrize("fmt", FORMATS)
def test_only_the_new_name_is_profiled(vb, fmt):
    rng = np.random.default_rng(5)
    _, raw = _source(fmt, rng, 4099 * 3)
    src = vb.to_device(raw, np.uint8)
    out = vb.empty((3, 4224), OUT[fmt])
    vb.profile(True)
    vb.profile_reset()
    try:
        vb.unpack_channels(src, 4099, fmt, 3, out=out, plane_ld=4224)          # whole tiles and a tail
        vb.unpack_channels(src, 4099 * 3, fmt, 1, out=out, plane_ld=4099 * 3)  # one channel: the mono forms, still under the new name
        rep = vb.profile_report()
    finally:
        vb.profile(False)
    assert sorted(rep) == [NAMES[fmt]] and rep[NAMES[fmt]][1] == 2, sorted(rep)
    src.free(); out.free()


def test_errors_write_nothing(vb):
    n, channels, ld = 64, 4, 96
    src = vb.to_device(np.zeros(n * channels, np.int32))
    a = la.Arena(la.DeviceBackend(vb), "unpack_channels errors")
    a.output("planes", np.float64, channels, n, ld=ld)
    a.place()
    fn = vb.L.vbx_unpack_channels

    def call(s=src.ptr, count=n, fmt=PCM32, ch=channels, sel=(0, 1, 2, 3), n_sel=None, no_sel=False, out=None, pld=ld):
        sa = np.array(sel, dtype=np.int32)
        return fn(vb.ctx, s, count, fmt, ch, None if no_sel else sa.ctypes.data, len(sel) if n_sel is None else n_sel,
                  a["planes"] if out is None else out, pld)
    assert call(fmt=0) == E_INVALID and call(fmt=6) == E_INVALID                       # an unknown format
    assert call(ch=0) == E_INVALID and call(ch=-1) == E_INVALID                        # channels < 1
    assert call(n_sel=0) == E_INVALID and call(sel=(0, 1, 2, 3, 0), n_sel=5) == E_INVALID      # n_sel outside [1, channels]
    assert call(no_sel=True) == E_INVALID
    assert call(sel=(0, 1, 1)) == E_INVALID and call(sel=(2, 0, 2, 1)) == E_INVALID    # a repeated channel
    assert call(sel=(0, 4)) == E_INVALID and call(sel=(-1, 0)) == E_INVALID            # a channel out of range
    assert call(pld=n - 1) == E_INVALID                                                # plane_ld < n_sample_frames
    assert call(s=None) == E_INVALID and fn(vb.ctx, src.ptr, n, PCM32, channels, np.arange(4, dtype=np.int32).ctypes.data, 4, None, ld) == E_INVALID
    assert call(s=src.ptr + 2) == E_INVALID                                            # an int32 source at 2 mod 4
    assert call(out=a["planes"] + 4) == E_INVALID                                      # a double destination at 4 mod 8
    assert call(fmt=PCM16, out=a["planes"] + 1) == E_INVALID and call(fmt=F32, out=a["planes"] + 2) == E_INVALID
    assert call(s=None, count=0, out=0, pld=0) == 0                                    # nothing to do
    assert call(count=0, sel=(0, 0)) == E_INVALID                                      # ... but a bad selection stays one
    out = a.finish(free=False)["planes"]
    assert la.unwritten(out).shape[0] == out.size
    assert call() == 0                                                                 # the context is usable afterwards
    out = a.finish()["planes"]
    assert np.array_equal(out, np.zeros((channels, n)))
    src.free()
