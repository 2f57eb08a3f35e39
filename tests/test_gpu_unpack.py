"""vbx_unpack_samples on a real MI355X: one channel of interleaved sample frames as the type the frame loop reads natively.  Every
comparison is BIT FOR BIT against numpy (uint64 / uint32 / uint16 views, so NaN payloads and the sign of zero count): 24- and
32-bit PCM are the correctly rounded quotients numpy.float64(s) / 8388607 and / 2147483647 -- numpy's float64 division is IEEE --
and PCM16, float and double are copies.  The outputs of the layout cases sit inside fenced arenas (tests/layout_arena.py)."""
import numpy as np
import pytest

import layout_arena as la

pytestmark = pytest.mark.gpu

E_INVALID = -1
PCM16, PCM24, PCM32, F32, F64 = 1, 2, 3, 4, 5
NAMES = {PCM16: "unpack_pcm16", PCM24: "unpack_pcm24", PCM32: "unpack_pcm32", F32: "unpack_f32", F64: "unpack_f64"}
OUT = {PCM16: np.int16, PCM24: np.float64, PCM32: np.float64, F32: np.float32, F64: np.float64}


def _pack24(s):
    """int32 values in [-2^23, 2^23) as packed 3-byte little-endian two's complement"""
    return np.ascontiguousarray(np.ascontiguousarray(s, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)


def _expected(fmt, vals):
    """what the selected samples (int / float array) become"""
    if fmt == PCM24:
        return vals.astype(np.float64) / np.float64(8388607.0)
    if fmt == PCM32:
        return vals.astype(np.float64) / np.float64(2147483647.0)
    return vals.copy()


def _source(fmt, rng, total):
    """`total` samples of the format: (typed values, their bytes as the library reads them)"""
    if fmt == PCM16:
        v = rng.integers(-32768, 32768, total).astype(np.int16)
    elif fmt == PCM24:
        v = rng.integers(-(1 << 23), 1 << 23, total).astype(np.int32)
        return v, _pack24(v)
    elif fmt == PCM32:
        v = rng.integers(-(1 << 31), 1 << 31, total).astype(np.int32)
    elif fmt == F32:
        v = rng.standard_normal(total).astype(np.float32)
    else:
        v = rng.standard_normal(total)
    return v, v.view(np.uint8).copy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _run(vb, fmt, raw, n, channels=1, channel=0, src_off=0):
    """unpack from a plain device buffer (the source starts src_off bytes in) into a plain device buffer"""
    src = vb.to_device(np.concatenate([np.zeros(src_off, np.uint8), raw]), np.uint8)
    out = vb.empty(max(n, 1), OUT[fmt])
    vb._check(vb.L.vbx_unpack_samples(vb.ctx, src.ptr + src_off, n, fmt, channels, channel, out.ptr))
    got = out.numpy()[:n]
    src.free(); out.free()
    return got


def test_pcm24_every_value(vb):
    s = np.arange(-(1 << 23), 1 << 23, dtype=np.int32)
    got = _run(vb, PCM24, _pack24(s), s.size)
    want = s.astype(np.float64) / np.float64(8388607.0)
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (bad.size, int(s[bad[0]]), got[bad[0]], want[bad[0]])
    assert got[0] < -1.0 and got[-1] == 1.0 and got[1 << 23] == 0.0 and not np.signbit(got[1 << 23])


def test_pcm32_edges_and_random(vb):
    edges = np.array([-(1 << 31), (1 << 31) - 1, 0, 1, -1, 2147483647, -2147483647], dtype=np.int64).astype(np.int32)
    rnd = np.random.default_rng(32).integers(-(1 << 31), 1 << 31, 1_000_000).astype(np.int32)
    s = np.concatenate([edges, rnd])
    got = _run(vb, PCM32, s.view(np.uint8), s.size)
    want = s.astype(np.float64) / np.float64(2147483647.0)
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (bad.size, int(s[bad[0]]), got[bad[0]], want[bad[0]])
    assert got[1] == 1.0 and got[5] == 1.0 and got[6] == -1.0 and got[0] < -1.0


def test_pcm16_every_value_is_what_pcm16_to_f64_reads(vb):
    s = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    got = _run(vb, PCM16, s.view(np.uint8), s.size)
    assert got.dtype == np.int16 and np.array_equal(got, s)
    # ... so the frame loop's PCM kernels divide the same integers: vbx_pcm16_to_f64 of the unpacked channel of a stereo source
    stereo = np.stack([s[::-1], s], axis=1)
    ch1 = _run(vb, PCM16, np.ascontiguousarray(stereo).view(np.uint8).reshape(-1), s.size, 2, 1)
    a, b = vb.pcm16_to_f64(ch1), vb.pcm16_to_f64(s)
    wa, wb = a.numpy(), b.numpy()
    a.free(); b.free()
    assert np.array_equal(_bits(wa), _bits(wb)) and np.array_equal(_bits(wb), _bits(s.astype(np.float64) / 32767.0))


@pytest.mark.parametrize("fmt", [F32, F64])
def test_floats_arrive_unchanged(vb, fmt):
    ut, ft = (np.uint32, np.float32) if fmt == F32 else (np.uint64, np.float64)
    tiny = np.finfo(ft).tiny
    words = [np.array(v, dtype=ft).view(ut) for v in (np.nan, -np.nan, -0.0, 0.0, np.inf, -np.inf, tiny / 4, -tiny / 1024, np.finfo(ft).max)]
    # NaNs with payloads, quiet and signalling
    pay = [0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFBFFFFF] if fmt == F32 else \
          [0x7FF8C0DEC0DE0001, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFF7FFFFFFFFFFFF]
    w = np.concatenate([np.array(words, dtype=ut).reshape(-1), np.array(pay, dtype=ut)])
    w = np.tile(w, 5)                                         # 65 values: whole groups and a tail
    for channels, channel in ((1, 0), (2, 1)):
        src = np.zeros((w.size, channels), dtype=ut)
        src[:, channel] = w
        got = _run(vb, fmt, np.ascontiguousarray(src).view(np.uint8).reshape(-1), w.size, channels, channel)
        assert np.array_equal(_bits(got), w), (fmt, channels)


@pytest.mark.parametrize("fmt", [PCM16, PCM24, PCM32, F32, F64])
def test_layouts_fenced(vb, fmt):
    rng = np.random.default_rng(100 + fmt)
    es = {PCM16: 2, PCM24: 3, PCM32: 4, F32: 4, F64: 8}[fmt]
    offsets = (0, 1, 2, 3) if fmt == PCM24 else (0, es)      # the other formats need their natural alignment: on and off 16 bytes
    for channels in (1, 2, 3):
        for n in (0, 1, 2, 3, 50_001):
            vals, raw = _source(fmt, rng, max(n, 1) * channels)
            for src_off in offsets:
                src = vb.to_device(np.concatenate([np.zeros(src_off, np.uint8), raw, np.zeros(16, np.uint8)]), np.uint8)
                for channel in range(channels):
                    for residue in (0, 8):
                        label = f"{NAMES[fmt]} channels {channels} channel {channel} n {n} source +{src_off} B, destination at {residue} mod 16"
                        a = la.Arena(la.DeviceBackend(vb), label)
                        a.output("out", OUT[fmt], 1, max(n, 4), residue=residue)
                        a.place()
                        vb._check(vb.L.vbx_unpack_samples(vb.ctx, src.ptr + src_off, n, fmt, channels, channel, a["out"]))
                        out = a.finish()["out"][0]                     # every fence byte intact: no overrun
                        want = _expected(fmt, vals.reshape(-1, channels)[:n, channel])
                        la.assert_same_bits(label, "out", out[:n], want.astype(OUT[fmt], copy=False))
                        assert la.unwritten(out[n:]).shape[0] == out.size - n, label      # nothing past element n
                src.free()


def test_errors(vb):
    src, out = vb.to_device(np.zeros(64, np.int32)), vb.empty(64)
    fn = vb.L.vbx_unpack_samples
    assert fn(vb.ctx, src.ptr, 8, 0, 1, 0, out.ptr) == E_INVALID and fn(vb.ctx, src.ptr, 8, 6, 1, 0, out.ptr) == E_INVALID
    assert fn(vb.ctx, src.ptr, 8, PCM32, 2, 2, out.ptr) == E_INVALID and fn(vb.ctx, src.ptr, 8, PCM32, 0, 0, out.ptr) == E_INVALID
    assert fn(vb.ctx, src.ptr, 8, PCM32, 2, -1, out.ptr) == E_INVALID
    assert fn(vb.ctx, None, 8, PCM32, 1, 0, out.ptr) == E_INVALID and fn(vb.ctx, src.ptr, 8, PCM32, 1, 0, None) == E_INVALID
    assert fn(vb.ctx, src.ptr + 2, 8, PCM32, 1, 0, out.ptr) == E_INVALID      # an int32 source at 2 mod 4
    assert fn(vb.ctx, src.ptr, 8, PCM24, 1, 0, out.ptr + 4) == E_INVALID      # a double destination at 4 mod 8
    assert fn(vb.ctx, None, 0, PCM32, 1, 0, None) == 0                        # nothing to do
    assert fn(vb.ctx, src.ptr, 8, PCM32, 1, 0, out.ptr) == 0                  # the context is usable afterwards
    assert np.array_equal(out.numpy()[:8], np.zeros(8))
    src.free(); out.free()


def test_every_launch_is_profiled(vb):
    rng = np.random.default_rng(5)
    vb.profile(True)
    vb.profile_reset()
    try:
        for fmt in NAMES:
            vals, raw = _source(fmt, rng, 1000)
            _run(vb, fmt, raw, 500, 2, 1)
        rep = vb.profile_report()
    finally:
        vb.profile(False)
    for name in NAMES.values():
        assert name in rep and rep[name][1] == 1, (name, sorted(rep))
