"""The f64 operations restated in numpy `longdouble` (x87 extended: 64-bit significand): the truth that tests/test_gpu_accuracy.py holds the
kernels AND the oracle to, and that tests/test_extended_truth_math.py checks against exact rational arithmetic.

Plain and slow on purpose: direct definitions, no FFT, no table the product shares.  Every DISCRETE decision (mel bins, statuses, index
clips, which sinc branch a point takes) is made in integers or on the f64 inputs exactly as oracle/vbx_oracle.c makes it; only the real
arithmetic is redone in long double.  pi is 4 atan(1) in long double, never the f64 constant; phases are reduced in integers before a
cosine is taken; sums are numpy's pairwise `np.sum` over a contiguous axis.  `reverse=True` takes every sum over the reversed terms:
the two results differ by the truth's own rounding error, which is how the CPU test shows that the truth resolves the oracle's.
The cases both tests run are in tests/accuracy_cases.py."""
import numpy as np

LD = np.longdouble
PI = 4 * np.arctan(LD(1))
U = 2.0 ** -53


def ld(a):
    return np.asarray(a, dtype=LD)


def _sum(a, reverse=False):
    """pairwise sum over the last axis, optionally over the reversed terms"""
    a = np.asarray(a, dtype=LD)
    return np.sum(np.ascontiguousarray(a[..., ::-1] if reverse else a), axis=-1)


def row_error(a, t):
    """e(A) = max_j |A_j - T_j| / max_j |T_j| of one row against its truth (a float)"""
    a, t = np.atleast_1d(ld(a)), np.atleast_1d(ld(t))
    return float(np.max(np.abs(a - t)) / np.max(np.abs(t)))


# ---- periodic.rs / waves.rs ----------------------------------------------------------------------------------------------------------

def autocorrelate(x, lags, reverse=False):
    """oracle/vbx_oracle.c:116: r[lag] = x[0] + sum_{i >= 1} x[i] x[i + lag] -- the fold's seed is x[0], not x[0]^2"""
    x = ld(x)
    n = x.size
    return np.array([x[0] + _sum(x[1:n - k] * x[1 + k:n], reverse) for k in range(lags)], dtype=LD)


def normalize(x):
    x = ld(x)
    return x * (LD(1) / np.max(np.abs(x)))


def rms(x, reverse=False):
    x = ld(x)
    return np.sqrt(_sum(x * x, reverse) / LD(x.size))


def preemphasis(x, factor):
    """oracle/vbx_oracle.c:102: backwards, x[k] += (2 pi factor) x[k + 1] with x[k + 1] already updated.  Rows [F, n] or one row."""
    x = ld(x).copy()
    filt = 2 * PI * LD(factor)
    last = x[..., -1].copy()
    for k in range(x.shape[-1] - 2, -1, -1):
        x[..., k] = x[..., k] + last * filt
        last = x[..., k].copy()
    return x


def interpolate_sinc(y, offset, nx, x, depth, reverse=False):
    """oracle/vbx_oracle.c:129 for one point: (status, value).  status 4 where the reference's index arithmetic leaves the slice."""
    y = ld(y)
    ylen = y.size
    x = float(x)
    fl = np.floor(x)
    nl = int(fl) if fl > 0.0 else 0
    nr = nl + 1
    if nx < 1:
        return 0, LD(np.nan)
    if x > float(nx):
        idx = offset + nx - 1
        return (4, LD(0)) if idx < 0 or idx >= ylen else (0, y[idx])
    if x < 0.0:
        return 0, y[0]
    if abs(x - float(nl)) < 1.0e-10:
        idx = offset + nl
        return (4, LD(0)) if idx < 0 or idx >= ylen else (0, y[idx])
    if abs(x - float(nr)) < 1.0e-10:
        idx = offset + nr
        return (4, LD(0)) if idx < 0 or idx >= ylen else (0, y[idx])
    phil = LD(x) - LD(nl)                                     # exact: x - floor(x) of an f64
    phir = LD(1) - phil
    md = int(depth)
    if offset + nr < md:
        md = 0 if offset + nr < 0 else offset + nr
    if offset + nl + md >= nx:
        md = nx - offset + nl - 1
    n = np.arange(md + 1)
    li = np.maximum(offset + nr - n, 0)
    if np.any(li >= ylen):
        return 4, LD(0)
    ri = np.minimum(np.maximum(offset + nl + n, 0), ylen - 1)
    al = PI * (phil + ld(n))
    ar = PI * (phir + ld(n))
    tl = y[li] * (np.sin(al) / al) * (LD(0.5) + LD(0.5) * np.cos(al / (phil + LD(md))))
    tr = y[ri] * (np.sin(ar) / ar) * (LD(0.5) + LD(0.5) * np.cos(ar / (phir + LD(md))))
    return 0, _sum(np.stack([tl, tr], axis=1).reshape(-1), reverse)


def resample_linear(x, ratio):
    """oracle/vbx_oracle.c:834 (the linear converter in front of find_formants at a resample_ratio), at any ratio.  The interpolation
    value v is the reference's own discrete stepping: advanced in f64 exactly as oracle/vbx_oracle.c:841-850 advances it
    (v += 1.0 / ratio, v -= 1.0 -- the rounding of 1 / ratio and of every step is part of WHICH point the converter evaluates, and the
    library's (li, frac) table is held to it bit for bit by tests/test_host_tables.py).  Only (right - left) * v + left is redone in
    long double.  tests/test_extended_truth_math.py checks that against exact rationals at a ratio whose inverse is no integer."""
    step = 1.0 / ratio
    x = ld(x)
    n = x.size
    m = int(np.ceil(ratio * n))
    nxt = 2
    left, right = x[0], (x[1] if n > 1 else LD(0))
    v, out = 0.0, np.zeros(m, LD)
    for k in range(m):
        while v >= 1.0:
            left, right = right, (x[nxt] if nxt < n else LD(0))
            nxt += 1
            v -= 1.0
        out[k] = (right - left) * LD(v) + left
        v += step
    return out


# ---- spectrum.rs -----------------------------------------------------------------------------------------------------------------------

def burg(x, p, reverse=False, reflection=False):
    """oracle/vbx_oracle.c:445 (LPC::lpc_praat_mut): p coefficients, no leading 1, negated at the end; None where den <= 0.
    reflection=True: (coefficients, the p reflection coefficients mu_i = 2 num_i / den_i)."""
    x = ld(x)
    n = x.size
    b1, b2, aa, co = np.zeros(n, LD), np.zeros(n, LD), np.zeros(p, LD), np.zeros(p, LD)
    mus = []
    b1[0] = x[0]
    b2[n - 2] = x[n - 1]
    b1[1:n - 1] = x[1:n - 1]
    b2[0:n - 2] = x[1:n - 1]
    for i in range(1, p + 1):
        m = n - i                                             # j - 1 in 0 .. n - i - 1
        num = _sum(b1[:m] * b2[:m], reverse)
        den = _sum(np.stack([b1[:m] * b1[:m], b2[:m] * b2[:m]], axis=1).reshape(-1), reverse)
        if den <= 0:
            return None
        co[i - 1] = 2 * num / den
        mus.append(co[i - 1])
        for j in range(1, i):
            co[j - 1] = aa[j - 1] - co[i - 1] * aa[i - j - 1]
        if i < p:
            aa[:i] = co[:i]
            m = n - i - 1                                     # j - 1 in 0 .. n - i - 2
            nb1 = b1[:m] - aa[i - 1] * b2[:m]                 # b2[j] of the reference's loop is still the old value,
            nb2 = b2[1:m + 1] - aa[i - 1] * b1[1:m + 1]       # b1[j] too: entry j - 1 is written before j is read
            b1[:m], b2[:m] = nb1, nb2
    return (-co, np.array(mus, dtype=LD)) if reflection else -co


def periodic_hanning(n):
    """the window find_formants applies (oracle/vbx_oracle.c:788): 0.5 (1 - cos(2 pi i / n))"""
    i = np.arange(n)
    return LD(0.5) * (1 - np.cos(2 * PI * ld(i) / LD(n)))


def dct(s, reverse=False):
    """oracle/vbx_oracle.c:872: c[k] = 2 sum_i s[i] cos(pi k (2 i + 1) / (2 n)), the phase reduced mod 4 n in integers"""
    s = ld(s)
    n = s.size
    tab = np.cos(PI * ld(np.arange(4 * n)) / LD(2 * n))
    k, i = np.arange(n)[:, None], np.arange(n)[None, :]
    return 2 * _sum(s[None, :] * tab[(k * (2 * i + 1)) % (4 * n)], reverse)


def dft_bins(x, k0, k1, reverse=False):
    """X[k] for k0 <= k < k1 by direct sums, the phase (k i) mod n reduced in integers: (re, im)"""
    x = ld(x)
    n = x.size
    ang = 2 * PI * ld(np.arange(n)) / LD(n)
    ct, st = np.cos(ang), np.sin(ang)
    i = np.arange(n, dtype=np.int64)[None, :]
    re, im = np.zeros(k1 - k0, LD), np.zeros(k1 - k0, LD)
    step = max(1, (1 << 20) // n)
    for a in range(k0, k1, step):
        k = np.arange(a, min(k1, a + step), dtype=np.int64)[:, None]
        idx = (k * i) % n
        re[a - k0:a - k0 + k.size] = _sum(x[None, :] * ct[idx], reverse)
        im[a - k0:a - k0 + k.size] = -_sum(x[None, :] * st[idx], reverse)
    return re, im


def mfcc(x, bins, reverse=False):
    """oracle/vbx_oracle.c:931 with the oracle's bins (oracle.mfcc_bins: integers): the rising half of a filter weighs |X|^2, the
    falling half |X|, both by i / width counted from the half's first bin; log10 clamped at 1e-10; the doubled DCT.
    Returns (coefficients, the smallest log10 filter energy before the clamp).  A filter whose halves are both at most one bin wide has
    only zero weights (i / width with i = 0): its energy is exactly 0 in any arithmetic, the clamp is certain, and it does not count
    towards that smallest energy (a fact of the integer bins: it happens where the mel points are less than two bins apart)."""
    bins = [int(b) for b in bins]
    nc = len(bins) - 2
    re, im = dft_bins(x, bins[0], max(bins[-1], bins[0] + 1), reverse)
    ns = re * re + im * im
    mag = np.sqrt(ns)
    en = np.zeros(nc, LD)
    for w in range(nc):
        w0, w1, w2 = bins[w], bins[w + 1], bins[w + 2]
        up = _sum(ns[w0 - bins[0]:w1 - bins[0]] * (ld(np.arange(w1 - w0)) / LD(max(w1 - w0, 1))), reverse)
        down = _sum(mag[w1 - bins[0]:w2 - bins[0]] * (ld(np.arange(w2 - w1)) / LD(max(w2 - w1, 1))), reverse)
        with np.errstate(divide="ignore"):
            en[w] = np.log10(up + down)
    live = [w for w in range(nc) if bins[w + 1] - bins[w] > 1 or bins[w + 2] - bins[w + 1] > 1]
    lo = float(np.min(en[live]))
    en = np.where(np.isnan(en) | (en < LD(1.0e-10)), LD(1.0e-10), en)
    return dct(en, reverse), lo


def to_resonance(roots, sample_rate):
    """oracle/vbx_oracle.c:647-679 on one row of roots: [count, 2] (frequency, bandwidth), sorted by frequency"""
    out = []
    mul = LD(sample_rate) / (PI * 2)
    for z in np.asarray(roots, dtype=np.complex128):
        zr, zi = LD(z.real), LD(z.imag)
        if z.imag >= 0.0:
            r, th = np.hypot(zr, zi), np.arctan2(zi, zr)
            if r > 1:
                ns = zr * zr + zi * zi                        # root.conj().inv()
                ir, ii = zr / ns, zi / ns
                r, th = np.hypot(ir, ii), np.arctan2(ii, ir)
            f, bw = mul * th, -2 * mul * np.log(r)
            if f > 50 and f < LD(sample_rate) * LD(0.5) - 50:
                out.append((f, bw))
    out.sort(key=lambda t: t[0])
    return np.array(out, dtype=LD).reshape(-1, 2)
