"""vbx_pitch_boersma_f64 in numpy float64: the executable form of the definition in include/voxbox_hip.h, rule by rule.

* `curve(xw)`: rule 1, the reference's lag curve (Q1 seed, Q2 normalisation over all lags, Q3 accumulated-phase lag window).
* `S(y, x, depth)`: rule 4, the interpolant with each side reading its own samples; `S_ld` is the same sum in np.longdouble.
* `brent(f, a, b)`: the reference's brent_maximize iteration (a minimiser), applied by the caller to -S (rule 7).
* `frame(xw, ...)`: rules 2-10 for one windowed frame -> FrameResult (row, count, status, which entries were selected, the
  refined lags, and the margin flag).

A frame is FLAGGED when a decision of the definition sits within 1e-9 of flipping, so that two correct float64 implementations may
disagree on it: a strict-peak comparison, a filter comparison (relative), the gap in s1 at the selection boundary, the gap between
two final strengths the sort orders."""
import math

import numpy as np

DEPTH_FIRST, DEPTH_REFINE = 30, 1200
FRAME_OK, FRAME_ERR_NAN = 0, 3
MARGIN = 1e-9


def hanning(n):
    """Window::<Hanning>::new(n): the phase accumulated by 1 / (n - 1), % 1.0."""
    out, ph, step = np.empty(n), 0.0, 1.0 / (float(n) - 1.0)
    for i in range(n):
        out[i] = 0.5 * (1.0 - math.cos(ph * (math.pi * 2.0)))
        ph = math.fmod(ph + step, 1.0)
    return out


def lag_window(n):
    """HanningLag::at_phase over the same accumulated phases (Q3)."""
    out, ph, step = np.empty(n), 0.0, 1.0 / (float(n) - 1.0)
    pi2 = math.pi * 2.0
    for i in range(n):
        v = ph * pi2
        out[i] = (1.0 - ph) * (2.0 / 3.0 + (1.0 / 3.0) * math.cos(v)) + (1.0 / pi2) * math.sin(v)
        ph = math.fmod(ph + step, 1.0)
    return out


_LAGW = {}


def curve(xw, lagw=None):
    """Rule 1.  xw: the windowed frame.  r[lag] = x[0] + sum_{i=1}^{N-lag-1} x[i] x[i+lag] (Q1), / max |r| over ALL lags, NaN never
    winning (Q2), / lag window (Q3)."""
    xw = np.asarray(xw, dtype=np.float64)
    n = xw.size
    if lagw is None:
        if n not in _LAGW:
            _LAGW[n] = lag_window(n)
        lagw = _LAGW[n]
    with np.errstate(all="ignore"):
        s = np.correlate(xw, xw, "full")[n - 1:]                 # S[lag] = sum_{i>=0} x[i] x[i+lag]
        r = (s - xw[0] * xw) + xw[0]
        amax = -1.0
        a = np.abs(r)
        fin = a[a > amax]                                        # NaN compares false
        if fin.size:
            amax = float(fin.max())
        return (r * (np.float64(1.0) / np.float64(amax))) / lagw


def _sum_terms(y, x, depth, dt, pi):
    nl = int(math.floor(x))
    phil = dt(x) - dt(nl)
    phir = dt(1.0) - phil
    D = min(depth, nl)
    if D <= 0:
        return dt(0.0)
    n = np.arange(D).astype(dt)
    yl = y[nl - np.arange(D)].astype(dt)
    yr = y[nl + 1 + np.arange(D)].astype(dt)
    al, ar = pi * (phil + n), pi * (phir + n)
    wl = dt(0.5) + dt(0.5) * np.cos(al / (phil + dt(D)))
    wr = dt(0.5) + dt(0.5) * np.cos(ar / (phir + dt(D)))
    return np.sum(yl * (np.sin(al) / al) * wl) + np.sum(yr * (np.sin(ar) / ar) * wr)


def _S(y, x, depth, dt, pi):
    if not x >= 0.0:
        return dt(y[0])
    nl = int(math.floor(x))
    if abs(x - nl) < 1e-10:
        return dt(y[nl])
    if abs(x - (nl + 1)) < 1e-10:
        return dt(y[nl + 1])
    with np.errstate(all="ignore"):
        return _sum_terms(y, x, depth, dt, pi)


def S(y, x, depth):
    """Rule 4 in float64."""
    return float(_S(y, float(x), depth, np.float64, np.float64(math.pi)))


_PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def S_ld(y, x, depth):
    """Rule 4 in np.longdouble (x itself is the float64 abscissa)."""
    return _S(y, float(x), depth, np.longdouble, _PI_LD)


def reflect(s):
    return 1.0 / s if s > 1.0 else s


def brent(f, a, b):
    """brent_maximize (src/periodic.rs:103-188): a minimiser of f over [a, b]; returns (x, f(x), evaluations)."""
    golden = 1. - 0.6180339887498948482045868343656381177203091798057628621
    sqrt_epsilon = 1.4901161193847656e-08
    eps = 2.220446049250313e-16
    tol = 1e-10
    v = a + golden * (b - a)
    fv = f(v)
    x = w = v
    fx = fw = fv
    evals = 1
    for _ in range(60):
        rng = b - a
        middle = (a + b) * 0.5
        tol_act = sqrt_epsilon * abs(x) + tol / 3.
        if abs(x - middle) + rng * 0.5 <= 2. * tol_act:
            break
        new_step = golden * (b - x) if x < middle else golden * (a - x)
        if abs(x - w) >= tol_act:
            t = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * t
            q = 2. * q - t
            if q > 0.:
                p = -p
            else:
                q = -q
            if abs(p) < abs(new_step * q) and p > q * (a - x + 2. * tol_act) and p < q * (b - x - 2. * tol_act):
                new_step = p / q
        if abs(new_step) < tol_act:
            new_step = tol_act if new_step > 0. else -tol_act
        t = x + new_step
        ft = f(t)
        evals += 1
        if ft <= fx:
            if t < x:
                b = x
            else:
                a = x
            v, w, x = w, x, t
            fv, fw, fx = fw, fx, ft
        else:
            if t < x:
                a = t
            else:
                b = t
            if ft <= fw or abs(w - x) < eps:
                v, w = w, t
                fv, fw = fw, ft
            elif ft <= fv or abs(v - x) < eps or abs(v - w) < eps:
                v = t
                fv = ft
    return x, fx, evals


class FrameResult:
    """row [kmax, 2], count, status; peaks: the kept peaks' k in L-order; selected: positions in L of the kept entries, in output
    order (len(peaks) is the unvoiced entry); xmid: their refined lags in output order (0.0 for the unvoiced entry); flagged."""

    def __init__(self, kmax):
        self.row = np.zeros((kmax, 2))
        self.count, self.status, self.flagged = 0, FRAME_OK, False
        self.peaks, self.x0, self.s1, self.selected, self.xmid, self.evals = [], [], [], [], [], 0


def _key(s):
    return math.inf if s != s else s


def frame(xw, sample_rate, threshold, fmin, fmax, kmax, y=None):
    """Rules 2-10 on one windowed frame (or on its curve y)."""
    if y is None:
        y = curve(xw)
    n = y.size
    H = n // 2
    res = FrameResult(kmax)
    near = False
    for k in range(1, H - 1):
        ym, yk, yp = float(y[k - 1]), float(y[k]), float(y[k + 1])
        if abs(yk - ym) < MARGIN or abs(yk - yp) < MARGIN:          # NaN: no margin, the comparison fails either way
            # only a comparison whose flip changes the answer: the other side must hold (or be near as well)
            if (ym < yk or abs(yk - ym) < MARGIN) and (yk > yp or abs(yk - yp) < MARGIN):
                near = True
        if not (ym < yk and yk > yp):
            continue
        with np.errstate(all="ignore"):
            dr = 0.5 * (yp - ym)
            d2r = 2.0 * yk - ym - yp
            dx = np.float64(dr) / np.float64(d2r)
            x0 = np.float64(k) + dx
            f0 = float(np.float64(sample_rate) / x0)
        if abs(f0 - fmin) <= MARGIN * abs(fmin) or abs(f0 - fmax) <= MARGIN * abs(fmax):
            near = True
        if fmin < f0 < fmax and abs(dx) <= 1.0:                    # |dx| < 0.5 but for cancellation in d2r
            res.peaks.append(k)
            res.x0.append(float(x0))
    res.s1 = [reflect(S(y, x0, DEPTH_FIRST)) for x0 in res.x0] + [float(threshold)]
    x0s = res.x0 + [0.0]
    total = len(x0s)
    m = min(kmax, total)
    keys = [_key(s) for s in res.s1]
    order = sorted(range(total), key=lambda i: (-keys[i], i))       # rank: larger s1 first, a tie to the earlier position
    if total > kmax and keys[order[m - 1]] - keys[order[m]] < MARGIN:
        near = True
    kept = sorted(order[:m])                                        # L-order
    freq, strength, xmids = [], [], []
    for i in kept:
        if x0s[i] == 0.0:
            freq.append(0.0); strength.append(res.s1[i]); xmids.append(0.0)
            continue
        xm, fx, ev = brent(lambda t: -S(y, t, DEPTH_REFINE), x0s[i] - 1.0, x0s[i] + 1.0)
        res.evals += ev
        freq.append(sample_rate / xm); strength.append(reflect(-fx)); xmids.append(xm)
    res.flagged = near
    if any(res.s1[i] != res.s1[i] for i in kept) or any(s != s for s in strength):
        res.status, res.count = FRAME_ERR_NAN, 0
        return res
    out = sorted(range(m), key=lambda j: (-strength[j], j))          # stable, descending
    ss = [strength[j] for j in out]
    if any(ss[j] - ss[j + 1] < MARGIN for j in range(m - 1)):
        res.flagged = True
    for pos, j in enumerate(out):
        res.row[pos] = (freq[j], strength[j])
    res.selected = [kept[j] for j in out]
    res.xmid = [xmids[j] for j in out]
    res.count = total
    return res


def frames_of(x, n_frames, frame_len, stride):
    x = np.asarray(x, dtype=np.float64)
    return np.lib.stride_tricks.as_strided(x, (n_frames, frame_len), (x.strides[0] * stride, x.strides[0]), writeable=False)


def pitch_boersma(x, n_frames, frame_len, stride, window, sample_rate, threshold, fmin, fmax, kmax):
    """The whole call: (cand [F, kmax, 2], count [F], status [F], results [F] of FrameResult)."""
    fr = frames_of(x, n_frames, frame_len, stride)
    cand = np.zeros((n_frames, kmax, 2))
    count, status, results = np.zeros(n_frames, np.int32), np.zeros(n_frames, np.int32), []
    for t in range(n_frames):
        with np.errstate(all="ignore"):
            xw = fr[t] * window if window is not None else np.array(fr[t])
        r = frame(xw, sample_rate, threshold, fmin, fmax, kmax)
        cand[t], count[t], status[t] = r.row, r.count, r.status
        results.append(r)
    return cand, count, status, results


def local_max_deficit(y, xmid):
    """max(S_ld(round(xmid)'s integer lag), S_ld(xmid +- 1e-3)) - S_ld(xmid): at most 1e-9 at a maximum Brent found (it stops
    within 2 tol_act ~ 1e-5 lags of a stationary point of a band-limited curve with |S''| of a few units: a deficit ~ 1e-10)."""
    k = int(round(xmid))
    here = S_ld(y, xmid, DEPTH_REFINE)
    around = max(S_ld(y, float(k), DEPTH_REFINE), S_ld(y, xmid - 1e-3, DEPTH_REFINE), S_ld(y, xmid + 1e-3, DEPTH_REFINE))
    return float(around - here), float(here)
