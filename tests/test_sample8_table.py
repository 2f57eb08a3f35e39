"""The arithmetic of the 8-bit sample formats, checked without a GPU: vbx_g711_table runs the SAME decode function the reader kernels
run (vbx_sample8.hpp), so the known answers, the CRCs, a pure-Python restatement of the ITU formulas and CPython's audioop (where it
can be imported) pin the kernels' integers; and unsigned 8-bit PCM's numpy reference, numpy.float64(b - 128) / 127, is shown to be
the correctly rounded quotient with exact rational arithmetic."""
import ctypes as C
import fractions
import os
import zlib

import numpy as np
import pytest

import sample8_cases as s8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = {s8.ULAW: {0x00: -32124, 0x80: 32124, 0x0f: -16764, 0x7f: 0, 0xff: 0},
         s8.ALAW: {0x55: -8, 0xd5: 8, 0x2a: -32256, 0xaa: 32256, 0x00: -5504}}
CRC = {s8.ULAW: 210008735, s8.ALAW: 2641774167}
ABS_SUM = {s8.ULAW: 1532928, s8.ALAW: 1564672}


@pytest.mark.parametrize("fmt", [s8.ULAW, s8.ALAW], ids=["ulaw", "alaw"])
def test_g711_table(pkg, fmt):
    t = pkg.g711_table(fmt)
    assert t.dtype == np.int16 and t.shape == (256,)
    for code, want in KNOWN[fmt].items():
        assert int(t[code]) == want, (hex(code), int(t[code]), want)
    assert zlib.crc32(t.astype("<i2").tobytes()) == CRC[fmt]
    assert int(np.abs(t.astype(np.int64)).sum()) == ABS_SUM[fmt]
    # the formulas of the header, restated in Python
    fn = s8.ulaw_value if fmt == s8.ULAW else s8.alaw_value
    assert [int(v) for v in t] == [fn(b) for b in range(256)]
    assert np.array_equal(t, s8.TABLE[fmt])
    # the range, the zero codes, the symmetry of the sign bit
    if fmt == s8.ULAW:
        assert int(t.min()) == -32124 and int(t.max()) == 32124 and sorted(np.nonzero(t == 0)[0].tolist()) == [0x7f, 0xff]
    else:
        assert int(t.min()) == -32256 and int(t.max()) == 32256 and not np.any(t == 0)
    assert np.array_equal(t[:128].astype(np.int32), -t[128:].astype(np.int32))
    try:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            import audioop
    except ImportError:
        audioop = None                                    # (removed from newer Pythons: this one comparison is left out)
    if audioop is not None:
        ref = (audioop.ulaw2lin if fmt == s8.ULAW else audioop.alaw2lin)(bytes(range(256)), 2)
        assert np.array_equal(np.frombuffer(ref, dtype=np.int16), t)


def test_g711_table_rejections(pkg):
    lib = pkg.load_library()
    out = (C.c_int16 * 256)(*([12345] * 256))
    for fmt in (0, 1, 6, 7, 16, 19, -1):
        assert lib.vbx_g711_table(fmt, out) == -1, fmt
        with pytest.raises(pkg.VoxBoxError):
            pkg.g711_table(fmt)
    assert lib.vbx_g711_table(17, None) == -1
    assert all(v == 12345 for v in out)                   # a rejected call writes nothing


def test_u8_reference_is_the_correctly_rounded_quotient():
    b = np.arange(256)
    got = s8.decode(s8.U8, b)
    assert got.dtype == np.float64
    assert np.array_equal(s8.bits(got), s8.bits(np.float64(1.0) * (b - 128).astype(np.float64) / np.float64(127.0)))
    for code in range(256):
        exact = fractions.Fraction(code - 128, 127)
        x = float(got[code])
        # float(Fraction) rounds the exact quotient to nearest-even: the IEEE division must give that double
        assert x == float(exact), code
        lo, hi = np.nextafter(x, -np.inf), np.nextafter(x, np.inf)
        err = abs(fractions.Fraction(x) - exact)
        assert err <= abs(fractions.Fraction(float(lo)) - exact) and err <= abs(fractions.Fraction(float(hi)) - exact), code
    assert got[0] == -128.0 / 127.0 and got[255] == 1.0 and got[128] == 0.0 and not np.signbit(got[128]) and got[1] == -1.0


def test_nearest_code_encoding_round_trips():
    """the tests' own encoder: every table value maps to a code of that value, and a sample between two values to the nearer one"""
    for fmt in (s8.ULAW, s8.ALAW):
        t = s8.TABLE[fmt]
        assert np.array_equal(t[s8.encode(fmt, t)], t)
        s = np.arange(-32768, 32768)
        d = np.abs(t[s8.encode(fmt, s)].astype(np.int64) - s)
        best = np.abs(t.astype(np.int64)[None, :] - s[:, None]).min(axis=1)
        assert np.array_equal(d, best)
    assert np.array_equal(s8.encode(s8.U8, np.array([-32768, -1, 0, 255, 256, 32767])), [0, 127, 128, 128, 129, 255])
    z = s8.silence(30)
    assert z.size == 30 and set(z.tolist()) == {0xff, 0xd5, 0x7f} and np.all(s8.TABLE[s8.ULAW][z[z != 0xd5]] == 0)
