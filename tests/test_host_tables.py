"""The builders of the device tables (csrc/vbx_host.cpp: window_dev_fill ... resample_fill), through vbx_internal_host_table, against
numpy restatements.  No device call.

Tables whose entries are single IEEE operations (slopes, resample recurrence, lag reciprocals, f32 rounding) must be EQUAL to the
float64 restatement.  Trigonometric tables are held to their closed form evaluated in numpy longdouble (x87 extended: the reference's
own error, ~2^-63, is negligible), with a bound per table derived in the test's docstring.  u = 2^-53 is the unit roundoff of double.
Every entry that the packing rules call padding must be exactly 0.0, and every size must be the size function's answer."""
import ctypes as C

import numpy as np
import pytest

WINDOW, LAG_F32, GOERTZEL, DFT2, MFMA, DCT, SLOPES, RESAMPLE = range(8)
LD = np.longdouble
TWO_PI = 2 * np.arccos(LD(-1))
ULP1 = 2.0 ** -52


def host_table(pkg, kind, ip, dp=None, dtypes=(np.float64,)):
    """-> (sub-tables, flags); asserts the size query and the fill agree and that nothing past the reported size is written"""
    fn = pkg.load_library().vbx_internal_host_table
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    ip = np.asarray(ip, np.int64)
    dp = None if dp is None else np.asarray(dp, np.float64)
    sub, flags = np.zeros(4, np.uint64), np.zeros(1, np.int32)
    assert fn(kind, ip.ctypes.data, None if dp is None else dp.ctypes.data, sub.ctypes.data, None, 0, flags.ctypes.data) == 0
    total = int(sum((int(b) + 15) & ~15 for b in sub))
    buf = np.full(total + 32, 0xA5, np.uint8)
    sub2 = np.zeros(4, np.uint64)
    assert fn(kind, ip.ctypes.data, None if dp is None else dp.ctypes.data, sub2.ctypes.data, buf.ctypes.data, total - 16, flags.ctypes.data) < 0
    assert np.all(buf == 0xA5)                                    # a buffer that is too small is refused, not written
    assert fn(kind, ip.ctypes.data, None if dp is None else dp.ctypes.data, sub2.ctypes.data, buf.ctypes.data, total, flags.ctypes.data) == 0
    assert np.array_equal(sub, sub2) and np.all(buf[total:] == 0xA5)
    out, off = [], 0
    for b, dt in zip(sub, dtypes):
        out.append(buf[off:off + int(b)].view(dt).copy())
        off += (int(b) + 15) & ~15
    assert all(int(b) == 0 for b in sub[len(dtypes):])
    return out, int(flags[0])


def plans(pkg, n):
    """the library's own plans for n-sample frames and the default band (13 filters, 100 - 8000 Hz at 48 kHz)"""
    bins, bad = pkg.mfcc_bins(n, 13, 100.0, 8000.0, 48000.0)
    assert not bad
    fn = pkg.load_library().vbx_internal_mfcc_table_plans
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    v = np.zeros(14, np.int32)
    assert fn(n, int(bins[0]), int(bins[-1] - bins[0]), v.ctypes.data) == 0
    return dict(zip("ok n1 n2 k2 mt ntd ntm src0 src1".split(), map(int, v[:9]))), dict(zip("ok n1 n2 nc tm".split(), map(int, v[9:])))


def cs(num, den):
    """(cos, sin)(2 pi num / den) for integer arrays, the phase reduced exactly, in longdouble"""
    ang = TWO_PI * (np.asarray(num, np.int64) % den).astype(LD) / LD(den)
    return np.cos(ang), np.sin(ang)


def err(a, ref):
    return float(np.max(np.abs(a.astype(LD) - ref))) if a.size else 0.0


# ---- single IEEE operations: equality ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 337, 1024, 1200])
def test_lag_window_reciprocals_and_f32_rounding(pkg, n):
    w = pkg.window_table(pkg.WINDOW_HANNING_LAG, n)
    (t,), flags = host_table(pkg, WINDOW, [pkg.WINDOW_HANNING_LAG, n])
    off = (n + 1) & ~1
    assert t.size == off + n
    assert np.array_equal(t[:n], w) and np.all(t[n:off] == 0.0)
    with np.errstate(divide="ignore"):
        r = 1.0 / w
    assert np.array_equal(t[off:], r)
    usable = bool(np.all(np.isfinite(r) & (np.abs(r) < 1e290) & (np.abs(r) > 1e-290)))
    assert flags == int(usable)
    (t32,), _ = host_table(pkg, LAG_F32, [n], dtypes=(np.float32,))
    assert t32.size == n and np.array_equal(t32, w.astype(np.float32))
    # the other windows are the plain table, no reciprocals, no flag
    for kind in (pkg.WINDOW_HANNING, pkg.WINDOW_HANNING_PERIODIC):
        (p,), f = host_table(pkg, WINDOW, [kind, n])
        assert f == 0 and np.array_equal(p, pkg.window_table(kind, n), equal_nan=True)


@pytest.mark.parametrize("n,k,lo,hi,sr", [(1200, 13, 100.0, 8000.0, 48000.0), (337, 13, 100.0, 8000.0, 48000.0), (1103, 20, 0.0, 8000.0, 44100.0),
                                          (32, 13, 100.0, 4000.0, 8000.0)])
def test_slopes(pkg, n, k, lo, hi, sr):
    """i / up on the rising side, i / down on the other: one IEEE division each.  (32, 13): neighbouring mel points share a bin, so
    some filters have up = 0 or down = 0 and write nothing."""
    bins, bad = pkg.mfcc_bins(n, k, lo, hi, sr)
    assert not bad
    bins = np.asarray(bins, np.int64)
    (t,), _ = host_table(pkg, SLOPES, [k] + list(bins))
    nb = int(bins[-1] - bins[0])
    assert t.size == 2 * max(nb, 1)
    ref = np.zeros((max(nb, 1), 2))
    for w in range(k):
        up, down = int(bins[w + 1] - bins[w]), int(bins[w + 2] - bins[w + 1])
        ref[bins[w] - bins[0]:bins[w] - bins[0] + up, 0] = np.arange(up, dtype=np.float64) / np.float64(up) if up else []
        ref[bins[w + 1] - bins[0]:bins[w + 1] - bins[0] + down, 1] = np.arange(down, dtype=np.float64) / np.float64(down) if down else []
    assert np.array_equal(t.reshape(-1, 2), ref)
    if (n, k) == (32, 13):
        assert np.any(np.diff(bins) == 0)


@pytest.mark.parametrize("ratio", [0.5, 1.0, 1.5, 64.0])
def test_resample_recurrence(pkg, ratio):
    """sample 0.10 Converter: value starts at 0 and grows by 1 / ratio per output; every whole unit moves the source index on"""
    n = 37
    m = int(pkg.load_library().vbx_resampled_len(n, ratio))
    (idx, frac), _ = host_table(pkg, RESAMPLE, [m], [ratio], dtypes=(np.int32, np.float64))
    assert idx.size == m and frac.size == m
    value, step, left = 0.0, 1.0 / ratio, 0                     # Python floats are IEEE doubles
    ri, rf = np.zeros(m, np.int32), np.zeros(m)
    for k in range(m):
        while value >= 1.0:
            left += 1
            value -= 1.0
        ri[k], rf[k] = left, value
        value += step
    assert np.array_equal(idx, ri) and np.array_equal(frac, rf)
    assert idx[0] == 0 and frac[0] == 0.0 and idx.max() <= n and np.all((frac >= 0.0) & (frac < 1.0))


# ---- trigonometric tables built in double ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 13, 64])
def test_dct_table(pkg, k):
    """h[kk][n] = cos(a), a = M_PI * kk * (2 n + 1) / (2 k) formed in double.  The bound is the one for tables built in double:
    |a| 2^-52 for the argument (|cos'| <= 1) + 2^-52 for the cosine's own evaluation and rounding."""
    (t,), _ = host_table(pkg, DCT, [k])
    assert t.size == k * k
    kk, n = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    arg = TWO_PI / 2 * kk.astype(LD) * (2 * n + 1).astype(LD) / LD(2 * k)
    d = np.abs(t.reshape(k, k).astype(LD) - np.cos(arg))
    bound = np.abs(arg) * ULP1 + ULP1
    worst = float(np.max(d / bound))
    print("dct k=%d: max |error| %.3g, max error / bound %.3f" % (k, float(d.max()), worst))
    assert np.all(d <= bound), worst


def test_goertzel_constants(pkg):
    """Bins [60, 260) of a 337-point DFT: the band crosses cos(w) = 0 (bin 84.25), so both forms appear.
    w = 2 M_PI (k % n) / n in double; cos(w) > 0: (4 sin^2(w / 2), +1), else (4 cos^2(w / 2), -1).  With the argument's error taken as
    |w| 2^-52 (the rule for tables built in double), d/dw 4 sin^2(w / 2) = 2 sin w gives 2 |w| 2^-52.  The entry is <= 2 (the form is
    chosen so that the squared half-angle function is <= 1 / 2) and carries libm's sin or cos (within 1 ulp: 2 u relative) twice in the
    square and the square's rounding, the factor 4 being exact: 5 u relative <= 5 2^-52 absolute.
    Bound: 2 |w| 2^-52 + 5 2^-52.  The sign must be exact wherever |cos w| exceeds the argument's error."""
    n, b_lo, nb = 337, 60, 200
    (t,), _ = host_table(pkg, GOERTZEL, [n, b_lo, nb])
    assert t.size == 2 * nb
    t = t.reshape(nb, 2)
    k = np.arange(b_lo, b_lo + nb) % n
    w = TWO_PI * k.astype(LD) / LD(n)
    pos = np.cos(w) > 0
    assert pos.any() and (~pos).any()
    sure = np.abs(np.cos(w)) > 1e-12
    assert np.array_equal(t[sure, 1], np.where(pos, 1.0, -1.0)[sure])
    ref = np.where(t[:, 1] > 0, 4 * np.sin(w / 2) ** 2, 4 * np.cos(w / 2) ** 2)
    d = np.abs(t[:, 0].astype(LD) - ref)
    bound = 2 * np.abs(w) * ULP1 + 5 * ULP1
    print("goertzel: max |error| %.3g, max error / bound %.3f" % (float(d.max()), float(np.max(d / bound))))
    assert np.all(d <= bound)
    (t0,), _ = host_table(pkg, GOERTZEL, [n, b_lo, 0])           # no bins: the two-entry placeholder stays zero
    assert t0.size == 2 and np.all(t0 == 0.0)


# ---- trigonometric tables built in long double and rounded once: one ulp of 1.0 ----------------------------------------------------------

def test_dft2_tables(pkg):
    """Plan of n = 1200.  ctab[i1][c]: cos(2 pi i1 c / n1) for c <= n1 / 2, then sin(2 pi i1 k1 / n1) for k1 = 1 ..; columns n1 .. nc are
    padding.  twid[j] = (cos, sin)(2 pi j / n).  Built in long double, rounded once: |error| <= 2^-53 + the long double's own 2^-63
    < 2^-52."""
    n = 1200
    _, pl = plans(pkg, n)
    assert pl["ok"] and pl["n1"] * pl["n2"] == n and pl["nc"] == (pl["n1"] + 3) & ~3
    n1, nc = pl["n1"], pl["nc"]
    (ctab, twid), _ = host_table(pkg, DFT2, [n, n1, nc], dtypes=(np.float64, np.float64))
    assert ctab.size == n1 * nc and twid.size == 2 * n
    ctab = ctab.reshape(n1, nc)
    ncos = n1 // 2 + 1
    i1 = np.arange(n1)[:, None]
    c = np.arange(n1)[None, :]
    k1 = np.where(c < ncos, c, c - ncos + 1)
    co, si = cs(i1 * k1, n1)
    assert err(ctab[:, :n1], np.where(c < ncos, co, si)) <= ULP1
    assert np.all(ctab[:, n1:] == 0.0)
    co, si = cs(np.arange(n), n)
    assert err(twid.reshape(n, 2)[:, 0], co) <= ULP1 and err(twid.reshape(n, 2)[:, 1], si) <= ULP1


@pytest.mark.parametrize("n", [400, 700, 1000])
def test_mfma_tables(pkg, n):
    """The four operand tables of the matrix-core MFCC kernel for the library's own plan of n: 400 = 25 x 16 and 700 = 25 x 28 (one direct
    and one mirror column tile; one and two row tiles, the second one partly padding), 1000 = 40 x 25 (two direct column tiles, n1 a
    multiple of 4).  Built in long double, rounded once: 2^-52.
    ctab[n1p][32 ntd]: cos columns k1 = c, then sin columns from 16 ntd on; rows >= n1 and columns with k1 >= n1 are padding.
    twd / twm[(m ntd + t) 4 + r][lane][2] = (cos, sin)(2 pi i2 k1 / n), i2 = 16 m + 4 r + (lane >> 4); k1 = 16 t + (lane & 15) for twd and
    n1 - (16 src_t + (lane & 15)) for twm; zero where i2 >= n2 or k1 outside [0, n1) (and the mirror of k1 = n1, kp = 0); 2 zeros of tail.
    wm[s][lane]: row = lane & 15 -> (k2 = row >> 1, p = row & 1), kk = 4 s + (lane >> 4) -> Re rows i2 = kk < 16 mt, Im rows after;
    p = 0: cos | sin, p = 1: -sin | cos of 2 pi i2 k2 / n2; zero where i2 >= n2 or k2 >= the plan's k2."""
    pl, _ = plans(pkg, n)
    assert pl["ok"] and pl["n1"] * pl["n2"] == n
    n1, n2, k2p, mt, ntd, ntm = (pl[k] for k in "n1 n2 k2 mt ntd ntm".split())
    (ctab, twd, twm, wm), _ = host_table(pkg, MFMA, [n] + [pl[k] for k in "n1 n2 k2 mt ntd ntm src0 src1".split()], dtypes=(np.float64,) * 4)
    n1p, nc = (n1 + 3) & ~3, 32 * ntd
    assert (ctab.size, twd.size, twm.size, wm.size) == (n1p * nc, mt * ntd * 512 + 2, mt * ntm * 512 + 2, 8 * mt * 64)
    # stage 1
    ctab = ctab.reshape(n1p, nc)
    i1, c = np.arange(n1p)[:, None], np.arange(nc)[None, :]
    is_sin = c >= 16 * ntd
    k1 = np.where(is_sin, c - 16 * ntd, c)
    live = (i1 < n1) & (k1 < n1)
    co, si = cs(i1 * k1, n1)
    assert err(ctab[live], np.broadcast_to(np.where(is_sin, si, co), live.shape)[live]) <= ULP1
    assert np.all(ctab[~live] == 0.0)

    def twiddles(tab, nt, k1_of):
        assert np.all(tab[-2:] == 0.0)
        tab = tab[:-2].reshape(mt, nt, 4, 64, 2) if nt else tab[:-2].reshape(0, 0, 4, 64, 2)
        m, t, r, lane = np.meshgrid(np.arange(mt), np.arange(nt), np.arange(4), np.arange(64), indexing="ij")
        i2, k1 = 16 * m + 4 * r + (lane >> 4), k1_of(t, lane & 15)
        live = (i2 < n2) & (k1 >= 0) & (k1 < n1)
        co, si = cs(i2 * np.where(live, k1, 0), n)
        assert err(tab[..., 0][live], co[live]) <= ULP1 and err(tab[..., 1][live], si[live]) <= ULP1
        assert np.all(tab[~live] == 0.0)
        return live
    twiddles(twd, ntd, lambda t, col: 16 * t + col)
    src = np.array([pl["src0"], pl["src1"]])
    twiddles(twm, ntm, lambda t, col: np.where(16 * src[np.minimum(t, 1)] + col >= 1, n1 - (16 * src[np.minimum(t, 1)] + col), -1))
    # stage 2
    s, lane = np.meshgrid(np.arange(8 * mt), np.arange(64), indexing="ij")
    row, kk = lane & 15, 4 * s + (lane >> 4)
    im = kk >= 16 * mt
    i2, k2, p = np.where(im, kk - 16 * mt, kk), row >> 1, row & 1
    live = (i2 < n2) & (k2 < k2p)
    co, si = cs(i2 * k2, n2)
    ref = np.where(p == 0, np.where(im, si, co), np.where(im, co, -si))
    wm = wm.reshape(8 * mt, 64)
    assert err(wm[live], ref[live]) <= ULP1
    assert np.all(wm[~live] == 0.0) and (~live).any()


def test_bad_parameters_are_refused(pkg):
    fn = pkg.load_library().vbx_internal_host_table
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    sub, flags = np.zeros(4, np.uint64), np.zeros(1, np.int32)
    for kind, ip, dp in ((DCT, [0], None), (DCT, [65], None), (99, [1], None), (RESAMPLE, [10], [0.0]), (RESAMPLE, [10], [float("nan")]),
                         (MFMA, [400, 25, 17, 1, 1, 1, 1, 0, 0], None), (DFT2, [1200, 7, 8], None), (SLOPES, [2, 5, 4, 6, 7], None)):
        ip = np.asarray(ip, np.int64)
        dp = None if dp is None else np.asarray(dp, np.float64)
        assert fn(kind, ip.ctypes.data, None if dp is None else dp.ctypes.data, sub.ctypes.data, None, 0, flags.ctypes.data) < 0
