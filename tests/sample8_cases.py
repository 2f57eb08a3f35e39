"""What the 8-bit sample formats mean, restated in numpy for the sample8 tests (VBX_SAMPLE_U8 / ULAW / ALAW: include/voxbox_hip.h),
and the recordings those tests share.  Nothing here asks the library: the G.711 tables come from the ITU formulas as the header
states them, unsigned 8-bit PCM is numpy.float64(b - 128) / 127 (numpy's float64 division is IEEE).

Realistic G.711 input is made from 16-bit audio without an encoder definition: every sample goes to the code whose table value is
nearest (numpy.searchsorted on the sorted table).  Every recording also holds all 256 codes and a stretch of digital silence -- runs
of 0xff, of 0xd5, and 0x7f and 0xff mixed -- so that all-zero and degenerate frames go through the comparisons."""
import os
import wave

import numpy as np

PCM16, F64 = 1, 5
U8, ULAW, ALAW = 16, 17, 18
FORMATS8 = (U8, ULAW, ALAW)
TAG = {U8: "u8", ULAW: "ulaw", ALAW: "alaw"}
OUT = {U8: np.float64, ULAW: np.int16, ALAW: np.int16}
GROUP = {U8: 2, ULAW: 8, ALAW: 8}                  # elements in a lane's 16 output bytes
SAME_AS = {U8: F64, ULAW: PCM16, ALAW: PCM16}      # the format whose call an 8-bit call must equal, on the decoded samples
TILE_BYTES = 8192


def ulaw_value(b):
    u = ~b & 0xff
    e, m = (u >> 4) & 7, u & 15
    mag = (((m << 3) + 0x84) << e) - 0x84
    return -mag if u & 0x80 else mag


def alaw_value(b):
    a = b ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    mag = (m << 4) + 8 if e == 0 else ((m << 4) + 0x108) << (e - 1)
    return mag if a & 0x80 else -mag


TABLE = {ULAW: np.array([ulaw_value(b) for b in range(256)], dtype=np.int16),
         ALAW: np.array([alaw_value(b) for b in range(256)], dtype=np.int16)}


def decode(fmt, codes):
    """what each byte becomes, as the plane's type"""
    codes = np.asarray(codes, dtype=np.uint8)
    if fmt == U8:
        return (codes.astype(np.float64) - np.float64(128.0)) / np.float64(127.0)
    return TABLE[fmt][codes]


def encode(fmt, s16):
    """the code whose value is nearest to each 16-bit sample (U8: the top byte, offset)"""
    s = np.asarray(s16, dtype=np.int64)
    if fmt == U8:
        return ((s >> 8) + 128).astype(np.uint8)
    t = TABLE[fmt].astype(np.int64)
    order = np.argsort(t, kind="stable")
    ts = t[order]
    i = np.clip(np.searchsorted(ts, s), 1, 255)
    i = np.where(np.abs(ts[i - 1] - s) <= np.abs(ts[i] - s), i - 1, i)
    return order[i].astype(np.uint8)


def silence(n):
    """digital silence of n codes: runs of 0xff, of 0xd5, and 0x7f / 0xff mixed"""
    k = n // 3
    mixed = np.where(np.arange(n - 2 * k) % 3 == 1, 0x7f, 0xff)
    return np.concatenate([np.full(k, 0xff), np.full(k, 0xd5), mixed]).astype(np.uint8)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def random_codes(rng, n):
    """n random codes with all 256 first (where they fit) and a stretch of silence inside"""
    c = rng.integers(0, 256, n).astype(np.uint8)
    if n >= 256:
        c[:256] = rng.permutation(256)
    if n >= 1024:
        c[400:400 + 384] = silence(384)
    return c


def golden_pcm16(golden_dir, name="short_sample.wav"):
    with wave.open(os.path.join(golden_dir, name), "rb") as w:
        assert w.getsampwidth() == 2
        a = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)
        return a.reshape(-1, w.getnchannels())[:, 0].copy()


def recording(fmt, n, speech, seed=0, silent=(0.45, 0.12)):
    """n codes of format fmt: 16-bit speech (tiled to length) encoded to the nearest codes, a stretch of digital silence inside (from
    the fraction silent[0] of the length on, silent[1] of it long), and all 256 codes once in front of it"""
    rng = np.random.default_rng(seed)
    s = np.resize(np.asarray(speech, dtype=np.int16), n)
    c = encode(fmt, s)
    a, ln = int(silent[0] * n), max(int(silent[1] * n), 3)
    c[a:a + ln] = silence(ln)[:max(0, min(ln, n - a))]
    if a >= 256:
        c[a - 256:a] = rng.permutation(256).astype(np.uint8)
    return c


def tile_frames(channels):
    """sample frames per LDS tile of the multi-channel readers at one byte per sample"""
    return (TILE_BYTES // channels) & ~15 if channels <= TILE_BYTES // 16 else 0
