"""Is the truth itself true?  tests/extended_truth.py (the f64 operations in long double) is what tests/test_gpu_accuracy.py holds the
kernels to at rounding level, so it is checked here, without a GPU:

  * exactly, at tiny sizes: autocorrelation, Burg and Levinson are rational arithmetic -- the long-double results sit within 64 long-double
    ulps of the value `fractions.Fraction` gives;
  * at the shapes the GPU test uses (tests/accuracy_cases.py): the truth computed with every sum taken forward and reversed agrees to
    better than E_O / 16, E_O being the oracle's own error against it -- the truth resolves the error it is asked to judge;
  * the inputs are well conditioned (conditions, not measurements): at most one row in eight of a case is excluded (MFCC next to the log10
    clamp, Burg where long double cannot arbitrate), and E_O <= 1e-13 on every case.  E_O of every case goes to a JSON file
    (profiles/accuracy/canary.json is the committed copy): inputs changed into an ill-conditioned regime fail here before a GPU is asked."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import accuracy_cases as ac
import extended_truth as xt
from lpc_exact_model import levinson

LD = np.longdouble
CANARY = {}


# ---- exact ---------------------------------------------------------------------------------------------------------------------------

def _frac(v):
    """a long double as the rational it is"""
    hi = float(v)
    lo = float(LD(v) - LD(hi))
    assert LD(v) - LD(hi) - LD(lo) == 0
    return Fraction(hi) + Fraction(lo)


def _within_ulps(got, exact, ulps=64):
    """|got - exact| <= ulps long-double ulps of the exact value (64-bit significand)"""
    if exact == 0:
        return _frac(got) == 0
    e = math.frexp(float(exact))[1]                           # |exact| in [2^(e-1), 2^e)
    return abs(_frac(got) - exact) <= ulps * Fraction(2) ** (e - 64)


def _burg_exact(x, p):
    """oracle/vbx_oracle.c:445 in rationals"""
    n = len(x)
    b1, b2, aa, co = [Fraction(0)] * n, [Fraction(0)] * n, [Fraction(0)] * p, [Fraction(0)] * p
    b1[0], b2[n - 2] = x[0], x[n - 1]
    for j in range(2, n):
        b1[j - 1] = x[j - 1]
        b2[j - 2] = x[j - 1]
    for i in range(1, p + 1):
        num = sum(b1[j - 1] * b2[j - 1] for j in range(1, n - i + 1))
        den = sum(b1[j - 1] * b1[j - 1] + b2[j - 1] * b2[j - 1] for j in range(1, n - i + 1))
        co[i - 1] = 2 * num / den
        for j in range(1, i):
            co[j - 1] = aa[j - 1] - co[i - 1] * aa[i - j - 1]
        if i < p:
            for j in range(1, i + 1):
                aa[j - 1] = co[j - 1]
            for j in range(1, n - i):
                b1[j - 1] = b1[j - 1] - aa[i - 1] * b2[j - 1]
                b2[j - 1] = b2[j] - aa[i - 1] * b1[j]
    return [-c for c in co]


def _levinson_exact(r):
    """src/spectrum.rs:63-84 in rationals"""
    p1 = len(r)
    a = [Fraction(1)] + [Fraction(0)] * (p1 - 1)
    err = r[0]
    for i in range(1, p1):
        acc = r[i] + sum(a[j] * r[i - j] for j in range(1, i))
        k = -acc / err
        t = list(a)
        a[i] = k
        for j in range(1, i):
            a[j] = t[j] + k * t[i - j]
        err = err * (1 - k * k)
    return a


def test_autocorrelation_is_exact_at_64_samples():
    x = np.random.default_rng(64).uniform(-1, 1, 64)
    xf = [Fraction(float(v)) for v in x]
    for reverse in (False, True):
        got = xt.autocorrelate(x, 64, reverse)
        for k in range(64):
            exact = xf[0] + sum(xf[i] * xf[i + k] for i in range(1, 64 - k))
            assert _within_ulps(got[k], exact), (k, reverse)


def test_burg_is_exact_at_24_samples_order_4():
    rng = np.random.default_rng(24)
    for trial in range(4):
        x = rng.uniform(-1, 1, 24)
        exact = _burg_exact([Fraction(float(v)) for v in x], 4)
        for reverse in (False, True):
            got = xt.burg(x, 4, reverse)
            assert all(_within_ulps(got[j], exact[j]) for j in range(4)), (trial, reverse)


def test_levinson_is_exact_at_order_4():
    rng = np.random.default_rng(4)
    for trial in range(4):
        x = rng.uniform(-1, 1, 40)
        r = np.array([np.dot(x[:40 - k], x[k:]) for k in range(5)])
        exact = _levinson_exact([Fraction(float(v)) for v in r])
        got = levinson(r[None, :], LD)[0]
        assert all(_within_ulps(got[j], exact[j]) for j in range(5)), trial


def _resample_exact(x, ratio):
    """oracle/vbx_oracle.c:834-851 in rationals: the interpolation value stepped in f64 as there, the interpolation itself exact"""
    n, m = len(x), int(math.ceil(ratio * len(x)))
    at = lambda i: x[i] if i < n else Fraction(0)
    left, right, nxt, v, step, out = at(0), at(1), 2, 0.0, 1.0 / ratio, []
    for _ in range(m):
        while v >= 1.0:
            left, right, nxt, v = right, at(nxt), nxt + 1, v - 1.0
        out.append((right - left) * Fraction(v) + left)
        v += step
    return out


@pytest.mark.parametrize("n,ratio", [(23, 10000.0 / 44100.0), (40, 10000.0 / 48000.0), (9, 1.5), (16, 0.25), (2, 64.0 / 3.0)])
def test_resampling_is_exact_at_ratios_whose_inverse_is_no_integer(oracle, n, ratio):
    """The long-double converter against exact rationals, its length and its sampling points against the oracle's: down by the example's
    10000 / 44100, up by 3 / 2 (the last outputs interpolate towards the zero past the frame).  Three roundings at 2^-64 with M = max |x|:
    right - left (at most 2 M), its product with v < 1 (at most 2 M), the sum (at most M): within 5 * 2^-64 M of the exact value (an
    output may be far smaller than M: ulps of the value itself would not be a bound)."""
    x = np.random.default_rng(n).uniform(-1, 1, n)
    got, exact = xt.resample_linear(x, ratio), _resample_exact([Fraction(float(v)) for v in x], ratio)
    assert got.size == len(exact) == oracle.resampled_len(n, ratio) and got.size >= 2
    bound = 5 * Fraction(2) ** -64 * Fraction(float(np.max(np.abs(x))))
    assert all(abs(_frac(got[k]) - exact[k]) <= bound for k in range(got.size))
    assert np.max(np.abs(oracle.resample_linear(x, ratio) - np.array([float(e) for e in exact]))) <= 2.0 ** -52
    if ratio > 1.0:
        assert exact[-1] != x[-1] and abs(exact[-1]) < abs(Fraction(float(x[-1])))      # between the last sample and the zero after it


def test_the_all_bins_case_needs_every_bin_of_the_half_spectrum(oracle):
    c = ac.BY_ID["mfcc-1000-all-bins"]
    b = ac.bins_of(oracle, c)
    assert b[0] == 0 and c.n // 2 <= b[-1] <= c.n


# ---- resolution and conditions at the GPU test's shapes --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def speech():
    return ac.host_speech()


def _conditions(name, e_o, e_rev):
    CANARY[name] = e_o
    assert e_rev < e_o / 16, (name, "forward and reversed sums differ by", e_rev, "the oracle's error is", e_o)
    assert e_o <= 1e-13, (name, e_o)


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.id)
def test_truth_resolves_the_oracle_and_inputs_are_well_conditioned(oracle, speech, case):
    X = ac.frames(case, speech, oracle)
    want = ac.rows(case)
    assert want[0] == 0 and want[-1] == case.F - 1 and len(want) <= (3 if case.n >= 2048 else 12)
    assert X[-1, 0] != 0.0                                   # the fold's seed counts on the last row
    keep, out, e_o, truth = ac.compared_rows(oracle, case, X)
    assert len(out) <= len(want) // 8, (case, "excluded rows", out)
    e_rev = max(xt.row_error(ac.truth_row(oracle, case, X, f, reverse=True)[0], truth[f]) for f in keep)
    _conditions(case.id, max(e_o.values()), e_rev)


@pytest.fixture(scope="module")
def fused_stream():
    import importlib
    import __graft_entry__ as g
    g.load_package()
    return importlib.import_module(g.PKG_NAME + ".synth").synth_speech(ac.FUSED_SAMPLES, sample_offset=ac.SPEECH_OFFSET)


@pytest.mark.parametrize("case", ac.FUSED_CASES, ids=lambda c: c.id)
def test_fused_mfcc_truth_resolves_the_oracle_and_inputs_are_well_conditioned(oracle, speech, fused_stream, case):
    """The same three conditions for the fused frame loop's MFCC cases (tests/test_gpu_accuracy.py::test_fused_mfcc): rows of the windowed
    stretch, 16-bit and float32 samples widened exactly."""
    assert np.array_equal(fused_stream[:speech.size], speech)                      # the fixture's own samples, continued
    up, wide = ac.fused_audio(case, fused_stream)
    assert wide.size == (case.F - 1) * case.hop + case.n <= fused_stream.size
    if case.sample == "pcm16":
        assert up.dtype == np.int16 and 32000 < np.abs(up.astype(np.int32)).max() <= 32767
    if case.sample == "f32":
        assert up.dtype == np.float32 and not np.array_equal(wide, fused_stream[:wide.size] * 40.0)
    X = ac.fused_frames(case, wide, oracle)
    want = ac.rows(case)
    assert want[0] == 0 and want[-1] == case.F - 1 and len(want) == (3 if case.n >= 2048 else 12)
    keep, out, e_o, truth = ac.compared_rows(oracle, case, X)
    assert len(out) <= len(want) // 8, (case, "excluded rows", out)
    e_rev = max(xt.row_error(ac.truth_row(oracle, case, X, f, reverse=True)[0], truth[f]) for f in keep)
    _conditions(case.id, max(e_o.values()), e_rev)


@pytest.mark.parametrize("depth", [30, 1200])
def test_sinc_truth(oracle, speech, depth):
    y, offset, nx, xs = ac.sinc_case(oracle, speech)
    fwd, rev, orc = [], [], []
    for x in xs:
        st, v = xt.interpolate_sinc(y, offset, nx, x, depth)
        so, vo = oracle.interpolate_sinc(y, offset, nx, x, depth)
        assert st == so == 0
        fwd.append(v); orc.append(vo); rev.append(xt.interpolate_sinc(y, offset, nx, x, depth, reverse=True)[1])
    scale = LD(np.max(np.abs(y)))
    fwd = np.array(fwd, dtype=LD)
    _conditions(f"sinc-depth{depth}", float(np.max(np.abs(xt.ld(orc) - fwd)) / scale),
                float(np.max(np.abs(np.array(rev, dtype=LD) - fwd)) / scale))


def test_small_operation_truths(oracle, speech):
    d = ac.small_inputs(speech)
    CANARY["normalize"] = max(xt.row_error(oracle.normalize(r), xt.normalize(r)) for r in d["normalize"])
    for n, rows in d["dct"].items():
        _conditions(f"dct-{n}", max(xt.row_error(oracle.dct(r), xt.dct(r)) for r in rows),
                    max(xt.row_error(xt.dct(r, True), xt.dct(r)) for r in rows))
    for n, rows in d["frames"].items():
        _conditions(f"rms-{n}", max(xt.row_error(oracle.rms(r), xt.rms(r)) for r in rows),
                    max(xt.row_error(xt.rms(r, True), xt.rms(r)) for r in rows))
        CANARY[f"preemphasis-{n}"] = max(xt.row_error(oracle.preemphasis(r, 0.1), xt.preemphasis(r, 0.1)) for r in rows)
    e = 0.0
    for r in d["roots"]:
        t, o = xt.to_resonance(r, ac.SR), oracle.to_resonance(r, ac.SR)
        assert t.shape == o.shape
        e = max(e, xt.row_error(o.reshape(-1), t.reshape(-1)))
    CANARY["to_resonance"] = e
    for k in ("normalize", "to_resonance", "preemphasis-100", "preemphasis-1200", "preemphasis-4096"):
        assert CANARY[k] <= 1e-13, (k, CANARY[k])             # no sums here: nothing to reverse


def test_the_guard_case_holds_rows_the_one_pass_recursion_gets_wrong(oracle):
    """tests/test_gpu_accuracy.py::test_one_pass_guard_against_the_truth is sensitive to a guard that lets frames through: among its
    compared rows (oracle within 1e-13 of the truth) the numpy model of the one-pass recursion is more than BF_TARGET from the truth on
    at least three, all of which the model's guard hands on; and where the guard trusts the recursion, it is inside the target."""
    from burg_one_pass_model import TARGET, burg_one_pass, parity_metric
    X, keep, truth = ac.guard_case(oracle)
    assert len(keep) >= 40, len(keep)
    co, trusted = burg_one_pass(X[keep], 12)
    d = parity_metric(co, np.array([np.asarray(truth[f], dtype=np.float64) for f in keep]))
    assert int(np.sum(d > TARGET)) >= 3, np.sort(d)[-5:]
    assert not np.any(trusted & (d > TARGET)), d[trusted].max()


def test_zz_canary_file(tmp_path):
    """Runs last in this file: E_O of every case, written out (into the directory VBX_TEST_REPORT_DIR names, when it names one)."""
    out = os.environ.get("VBX_TEST_REPORT_DIR")
    path = os.path.join(out if out and os.path.isdir(out) else str(tmp_path), "accuracy_canary.json")
    with open(path, "w") as fh:
        json.dump({"oracle_error_against_long_double": CANARY, "bound": 1e-13}, fh, indent=1, sort_keys=True)
    assert max(CANARY.values()) <= 1e-13, max(CANARY, key=CANARY.get)
