"""Assertions of GPU rows against the CPU oracle, shared by the parity tests (tests/test_gpu_parity.py, tests/test_gpu_f32.py)
and the layout tests (tests/test_gpu_layouts.py), so that the two cannot drift.  Tolerances are the project's: rel_close 1e-6
(SURVEY 8d), Hz 1e-4 relative, counts and statuses exact; the reference-faithful f32 forms EQUAL the f32 restatement bit for bit.
Every function looks at EVERY row it is given."""
import numpy as np

from conftest import rel_close


# ---- f64 ---------------------------------------------------------------------------------------------------------------------

def autocorrelate_rows(oracle, xw, lags, r, what=""):
    for f in range(xw.shape[0]):
        exp = oracle.autocorrelate(xw[f], lags)
        assert np.all(rel_close(r[f], exp)), (what, f, np.max(np.abs(r[f] - exp)))


def autocorr_lpc_rows(oracle, xw, p, norm, r, a, what="", lpc=True):
    for f in range(xw.shape[0]):
        er = oracle.autocorrelate(xw[f], p + 1)
        if norm:
            er = oracle.normalize(er)
        assert np.all(rel_close(r[f], er)), (what, f, "r")
        if lpc:
            ea = oracle.lpc(er, p)
            assert np.all(rel_close(a[f], ea)), (what, f, "lpc", np.max(np.abs(a[f] - ea)))


def burg_rows(oracle, xw, p, co, st, what=""):
    """Statuses exact; coefficient rows of status-0 frames rel_close, the others zero."""
    for f in range(xw.shape[0]):
        es, ec = oracle.lpc_burg(xw[f], p)
        assert st[f] == es, (what, f)
        if es == 0:
            assert np.all(rel_close(co[f], ec)), (what, f, np.max(np.abs(co[f] - ec)))
        else:
            assert np.all(co[f] == 0.0), (what, f)


def mfcc_rows(oracle, xw, nc, lo, hi, sr, m, st, what=""):
    for f in range(xw.shape[0]):
        es, em = oracle.mfcc(xw[f], nc, lo, hi, sr)
        assert st[f] == es, (what, f)
        if es == 0:
            assert np.all(rel_close(m[f], em)), (what, f, np.max(np.abs(m[f] - em)))


def find_roots_rows(oracle, polys, roots, st, what=""):
    """Status exact; every root of the oracle's find_roots_mut is among the row's within 1e-7 (a conjugate pair may come in either
    order: the quadratic tail orders it by the sign of rounding noise).  Returns the number of status-0 rows."""
    ok = 0
    for f in range(polys.shape[0]):
        es, er = oracle.find_roots_mut(polys[f])
        assert st[f] == es, (what, f, st[f], es)
        if es != 0:
            continue
        ok += 1
        g = np.asarray(roots[f], dtype=np.complex128)
        assert all(np.min(np.abs(g - r)) <= 1e-7 * max(1.0, abs(r)) for r in er), (what, f, g, er)
    return ok


def find_roots_f32_rows(oracle, P, r, st, what=""):
    """The Complex<f32> instantiation on real-coefficient polynomials P [F, len]: status equal to the f32 oracle's, the same
    number of roots, and every GPU root a root of the polynomial to f32 accuracy (conditioning-independent residual check;
    discovery order can differ when two Laguerre limits are rounding-close).  Returns the number of status-0 rows."""
    ok = 0
    for f in range(P.shape[0]):
        es, er = oracle.find_roots_f32(P[f].astype(np.complex64))
        assert st[f] == es, (what, f)
        if es != 0:
            continue
        ok += 1
        g = r[f, :er.size].astype(np.complex128)
        pv = np.polyval(P[f, ::-1].astype(np.float64), g)
        scale = np.polyval(np.abs(P[f, ::-1]).astype(np.float64), np.abs(g).astype(np.float64))
        assert np.all(np.abs(pv) <= 2e-4 * scale), (what, f, np.abs(pv) / scale)
        assert np.sort_complex(g).size == np.sort_complex(er.astype(np.complex128)).size
    return ok


# ---- Sample = f32 ------------------------------------------------------------------------------------------------------------

def autocorrelate_f32_rows(oracle, x32, lags, r, what=""):
    assert r.dtype == np.float32
    assert np.array_equal(r, np.stack([oracle.autocorrelate_f32(f, lags) for f in x32])), what


def normalize_f32_rows(oracle, r, rn, what=""):
    assert np.array_equal(rn, np.stack([oracle.normalize_f32(row) for row in r])), what


def lpc_f32_rows(oracle, r, p, ac, kc=None, what=""):
    """LPC::lpc_mut at T = f32: coefficients (and reflection coefficients) equal the f32 restatement's, bit for bit."""
    assert ac.dtype == np.float32 and np.all(ac[:, 0] == 1.0)
    for f in range(r.shape[0]):
        ea, ek = oracle.lpc_f32(r[f], p)
        assert np.array_equal(ac[f], ea), (what, f)
        if kc is not None:
            assert np.array_equal(kc[f], ek), (what, f, "kc")


def burg_f32_rows(oracle, x32, p, co, st, what=""):
    assert co.dtype == np.float32
    for f in range(x32.shape[0]):
        es, ec = oracle.lpc_burg_f32(x32[f], p)
        assert st[f] == es, (what, f)
        if es == 0:
            assert np.array_equal(co[f], ec), (what, f, co[f], ec)


def pitch_f32_rows(oracle, x32, sr, thr, fmin, fmax, cand, cnt, st, what=""):
    """Pitched<f32, f32>::pitch: status and COUNT equal the f32 restatement's on every frame; the top candidate within 1e-4 in Hz
    and strength unless the restatement's two best are closer than 1e-3.  Returns (frames compared, of those with identical bits,
    voiced top candidates)."""
    assert cand.dtype == np.float32
    n_same_bits = n_cmp = voiced = 0
    for f in range(x32.shape[0]):
        es, ec, en = oracle.pitch_f32(x32[f], sr, thr, fmin, fmax)
        assert st[f] == es and cnt[f] == (en if es == 0 else 0), (what, f, st[f], es, cnt[f], en)
        if es != 0:
            continue
        tie = en > 1 and abs(ec[0, 1] - ec[1, 1]) < 1e-3
        if not tie:
            assert abs(cand[f, 0, 0] - ec[0, 0]) <= 1e-4 * abs(ec[0, 0]) + 1e-12 and abs(cand[f, 0, 1] - ec[0, 1]) <= 1e-4, (what, f, cand[f, 0], ec[0])
            n_cmp += 1
            n_same_bits += int(np.float32(ec[0, 0]) == cand[f, 0, 0] and np.float32(ec[0, 1]) == cand[f, 0, 1])
            voiced += int(cand[f, 0, 0] > 0)
    return n_cmp, n_same_bits, voiced


def rounded_once(wide, f64_result, what=""):
    """A *_f32_wide result is the f64 entry point's on the widened frames, rounded to f32 once."""
    assert wide.dtype == np.float32 and np.array_equal(wide, np.asarray(f64_result).astype(np.float32)), what
