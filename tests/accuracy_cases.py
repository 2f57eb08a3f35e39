"""The cases of the accuracy tests: tests/test_extended_truth_math.py (CPU: is the truth good enough, are the inputs well conditioned) and
tests/test_gpu_accuracy.py (GPU: the kernels against the truth) run THE SAME list on the same rows.

Frames: Hanning-windowed synthetic speech (the voiced glide of the stream the other GPU tests use) and, as the last row of every batch, one
rectangular noise frame: x[0] != 0 there, so the seed of the reference's autocorrelation fold counts.  The MFCC frames are scaled by 40,
as tests/test_gpu_parity.py scales them: every filter's energy is then well above the log10 clamp.

Batch sizes: one frame more than the kernel's frames per block, so the last wavefront (or block) is partial: 17 for the few-lag kernel and
the one-pass Burg (9 at frames of up to 512 samples), 64 / G + 1 for the direct Burg; the kernels that take one frame per block get 6 frames,
3 from 2048 samples up.  Truth is computed for at most 12 rows of a batch (3 from 2048 samples up), the first and the last always."""
import numpy as np

import extended_truth as xt

SR = 48000.0
SPEECH_SAMPLES, SPEECH_OFFSET = 2 * 48000, 2 * 48000       # seconds 2..4 of the stream: voiced


class Case:
    def __init__(self, id, family, n, F, ctx_env=None, env=None, kernels=(), form=None, rect=False, cls=1, **p):
        self.id, self.family, self.n, self.F, self.p = id, family, n, F, p
        self.ctx_env, self.env, self.kernels, self.form, self.rect, self.cls = ctx_env or {}, env or {}, set(kernels), form, rect, cls

    def __repr__(self):
        return self.id


def fft_transform(n):
    """spectral_plan() of k_spectral.hip: the complex transform length that serves a frame of n samples"""
    return 1024 if n <= 1024 else 1200 if n <= 1200 else 2048 if n <= 2048 else 4096


def _one(n):
    return 3 if n >= 2048 else 6


def _ac(n, lags, kernel, F=None, **kw):
    return Case(f"autocorr-{n}x{lags}-{kernel}", "autocorr", n, F or _one(n), kernels={"autocorr_" + kernel}, lags=lags, **kw)


def _mf(tag, n, form, nc=13, lo=100.0, hi=8000.0, sr=SR, kernel="mfcc", **kw):
    return Case(f"mfcc-{n}-{tag}", "mfcc", n, _one(n), kernels={kernel}, form=form, nc=nc, lo=lo, hi=hi, sr=sr, **kw)


def _burg_fpb(n, p):
    """frames per block of the direct recursion (launch_burg_t, k_burg.hip): 64 / lane group"""
    if n > 4096:
        return 1
    if p <= 16 and n <= 512:
        return 4
    return 2 if n <= 1024 and p <= 32 else 1


def den_recursion(n, p):
    """the direct kernel's one-frame-per-wavefront form (G = 64) carries the denominator from order to order (k_burg.hip)"""
    return n <= 4096 and _burg_fpb(n, p) == 1


def den_recursion_bound(x, p):
    """First-order bound on the relative error of the denominators that k_burg.hip's G = 64 form carries from order to order,
         den' = (1 - mu^2) den - e_back^2 - e_front^2        instead of        den' = sum b1^2 + b2^2,
    from the TRUTH's reflection coefficients (never from GPU output).  One step rounds four times on terms no larger than den
    (1 - mu^2, its product with den, two FMAs): 4 eps den absolute.  A relative error d of den is also one of mu = 2 num / den, which
    moves (1 - mu^2) den by 2 mu^2 d den; together with the carried d (1 - mu^2) den that is (1 + mu^2) d den.  Relative to
    den' <= (1 - mu^2) den:
         d' <= (d + 4 eps) (1 + mu^2) / (1 - mu^2).
    On 48 kHz speech 1 - mu_1^2 ~ 0.02, so the first step alone multiplies by ~100 and the bound reaches ~3e-12 where the directly
    summed forms stay at 1e-16: the form's own arithmetic, not a defect (the kernel's header states eps / (1 - mu^2) per order and
    falls back to direct sums once 1 - mu^2 < 2^-20).  Returned: the largest d over the orders."""
    co, mu = xt.burg(x, p, reflection=True)
    mu = np.asarray(mu, dtype=np.float64)
    d = worst = 0.0
    for i in range(p - 1):
        d = (d + 4 * 2.0 ** -52) * (1 + mu[i] ** 2) / (1 - mu[i] ** 2)
        worst = max(worst, d)
    return worst


def _bd(n, p, tag=""):
    """direct recursion, forced for the shapes the one-pass form would take (the switch is read per call)"""
    return Case(f"burg-direct-{n}x{p}{tag}", "burg_direct", n, _burg_fpb(n, p) + 1, env={"VBX_BURG_DIRECT": "1"},
                kernels={"burg_long" if n > 4096 else "burg"}, order=p)


def _bf(n, p):
    return Case(f"burg-one-pass-{n}x{p}", "burg_fast", n, 9 if n <= 512 else 17, kernels={"burg_lags", "burg_recursion"}, cls=2,
                order=p)


MFMA = {"VBX_PITCH_MFMA": "1"}

CASES = [
    # -- autocorrelation: few-lag registers, matrix-core direct sums (one and two passes), the four FFT plans, long frames
    _ac(512, 13, "fewlags", F=17), _ac(100, 7, "fewlags", F=17), _ac(1200, 13, "fewlags", F=17),
    _ac(1280, 257, "tiles", ctx_env=MFMA), _ac(1281, 300, "tiles", ctx_env=MFMA),
    _ac(512, 512, "fft"), _ac(1024, 1024, "fft"), _ac(1103, 1103, "fft"), _ac(1200, 1200, "fft"),
    _ac(2047, 2047, "fft"), _ac(2048, 2048, "fft"), _ac(4095, 4095, "fft"), _ac(4096, 4096, "fft"),
    _ac(4097, 40, "long"),
    # -- MFCC, one case per form (run_mfcc, vbx_api.hip)
    _mf("fft", 1200, 1), _mf("fft", 2048, 1),
    _mf("interp", 1103, 2), _mf("interp", 3000, 2),
    _mf("czt", 1103, 3, hi=16000.0),
    _mf("czt-split", 1103, 3, hi=16000.0, ctx_env={"VBX_MFCC_CZT_SPLIT": "1"}), _mf("czt-split", 4000, 3, ctx_env={"VBX_MFCC_CZT": "1"}),      # too long for one chirp-z transform: split; interpolated by default
    _mf("mfma", 700, 4), _mf("mfma", 1280, 4),
    _mf("dft2", 1200, 5, ctx_env={"VBX_MFCC_DFT2": "1"}),
    _mf("goertzel", 509, 6), _mf("goertzel", 1200, 6, ctx_env={"VBX_MFCC_GOERTZEL": "1"}),
    _mf("long", 4097, 7, kernel="mfcc_long"),
    # 40 filters from 0 Hz to the Nyquist frequency (of tests/test_gpu_parity.py::test_mfcc): every bin up to n / 2 and beyond is needed
    _mf("all-bins", 1000, 3, nc=40, lo=0.0, hi=8000.0, sr=16000.0),
    # -- Burg: the direct recursion at every lane-group shape, then the one-pass shapes through both forms
    _bd(512, 12), _bd(100, 5), _bd(200, 17), _bd(513, 30), _bd(400, 62), _bd(2049, 13), _bd(4097, 12),
    _bd(1200, 12), _bd(2048, 8), _bd(1281, 16),
    _bf(512, 12), _bf(1200, 12), _bf(2048, 8), _bf(1281, 16),
    # -- find_formants at resample_ratio 1 / 4: the frame resampled inside the one-pass Burg's lag kernel (no window: find_formants has none)
    Case("burg-one-pass-resampled-1200x12", "burg_resampled", 1200, 17, kernels={"burg_lags_resampled"}, rect=True, cls=2, order=12, ratio=0.25),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

FAMILY_OF = {"autocorr": "autocorrelation", "mfcc": "mfcc", "burg_direct": "burg_direct", "burg_fast": "burg_direct"}
EST0 = np.array([[320.0, 1.0], [1440.0, 1.0], [2760.0, 1.0], [3200.0, 1.0]])


def host_speech():
    """the same stream from the host statement of the generator (within 1e-9 of the device's): what the CPU test conditions on"""
    import importlib
    import __graft_entry__ as g
    g.load_package()
    return importlib.import_module(g.PKG_NAME + ".synth").synth_speech(SPEECH_SAMPLES, sample_offset=SPEECH_OFFSET)


def frames(case, speech, oracle):
    k = CASES.index(case)
    base, hop = 1000 + 3001 * (k % 8), 997
    X = np.stack([speech[base + t * hop:base + t * hop + case.n] for t in range(case.F)])
    if not case.rect:
        X = X * oracle.window("hanning", case.n)
    if case.family == "mfcc":
        X = X * 40.0                                          # every filter's energy well above the log10 clamp at 1e-10
    X[-1] = np.random.default_rng(1000 * case.n + case.F).uniform(-0.8, 0.8, case.n)
    return np.ascontiguousarray(X)


def rows(case):
    cap = 3 if case.n >= 2048 else 12
    return sorted({int(round(v)) for v in np.linspace(0, case.F - 1, min(cap, case.F))})


def bins_of(oracle, case):
    return oracle.mfcc_bins(case.n, case.p["nc"], case.p["lo"], case.p["hi"], case.p["sr"])


def oracle_row(oracle, case, x):
    """the oracle's f64 row, its discrete results checked where it has any"""
    if case.family == "autocorr":
        return oracle.autocorrelate(x, case.p["lags"])
    if case.family == "mfcc":
        st, m = oracle.mfcc(x, case.p["nc"], case.p["lo"], case.p["hi"], case.p["sr"])
        assert st == 0, (case, st)
        return m
    if case.family == "burg_resampled":                      # find_formants: resample, periodic Hanning window, Burg
        st, _, _, co = oracle.find_formants(oracle.resample_linear(x, case.p["ratio"]), SR, case.p["order"], EST0)
        assert st == 0, (case, st)
        return co
    st, co = oracle.lpc_burg(x, case.p["order"])
    assert st == 0, (case, st)
    return co


_TRUTH = {}


def truth_row(oracle, case, X, f, reverse=False):
    """(truth row, the smallest log10 filter energy or None); cached: the CPU test asks for the same rows several times"""
    key = (case.id, f, reverse, X[f].tobytes()[:64])
    if key not in _TRUTH:
        if case.family == "autocorr":
            _TRUTH[key] = (xt.autocorrelate(X[f], case.p["lags"], reverse), None)
        elif case.family == "mfcc":
            _TRUTH[key] = xt.mfcc(X[f], bins_of(oracle, case), reverse)
        else:
            x = X[f]
            if case.family == "burg_resampled":
                x = xt.resample_linear(x, case.p["ratio"])
                x = x * xt.periodic_hanning(x.size)
            t = xt.burg(x, case.p["order"], reverse)
            assert t is not None, (case, f)
            _TRUTH[key] = (t, None)
    return _TRUTH[key]


def compared_rows(oracle, case, X):
    """The rows of a case that are compared, after the two exclusions the accuracy tests allow: an MFCC row whose smallest log10 filter
    energy is below 1e-3 (next to the clamp's discontinuity), a Burg row on which the ORACLE is more than 1e-10 from the truth (long
    double cannot arbitrate there).  Returns (kept rows, excluded rows, {row: oracle error}, {row: truth})."""
    keep, out, eo, tr = [], [], {}, {}
    for f in rows(case):
        t, lo = truth_row(oracle, case, X, f)
        e = xt.row_error(oracle_row(oracle, case, X[f]), t)
        if (case.family == "mfcc" and lo < 1e-3) or (case.family.startswith("burg") and e > 1e-10):
            out.append(f)
            continue
        keep.append(f); eo[f] = e; tr[f] = t
    return keep, out, eo, tr


# ---- the sinc sums and the small operations: fixed inputs, as tests/test_gpu_parity.py builds them ---------------------------------

def sinc_case(oracle, speech):
    """the lag curve of one windowed frame and the 300 interior points of test_interpolate_sinc_points: (y, offset, nx, xs)"""
    n = 1200
    x = speech[1000:1000 + n] * oracle.window("hanning", n)
    r = oracle.normalize(oracle.autocorrelate(x, n)) / oracle.window("hanning_lag", n)
    y = np.concatenate([r, np.zeros(n)])
    b = n // 2
    return y, -b - 1, 2 * b + 1, np.random.default_rng(1).uniform(b + 2, 2 * b, 300)


def small_inputs(speech):
    rng = np.random.default_rng(3)
    d = {"normalize": rng.standard_normal((7, 100)),
         "dct": {n: rng.uniform(-4.0, 9.0, (5, n)) for n in (13, 40, 64)},
         "frames": {n: np.stack([speech[4000 + 997 * t:4000 + 997 * t + n] for t in range(5)]) for n in (100, 1200, 4096)}}
    rng = np.random.default_rng(5)
    d["roots"] = rng.uniform(0.3, 1.3, (50, 12)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (50, 12)))
    return d


def guard_case(oracle, n=512, p=12):
    """Frames the one-pass Burg's guard exists for (tests/burg_one_pass_model.py: pure tones over noise floors down to 1e-9, resonators
    next to the unit circle, DC, ...), periodic Hanning window.  Compared: the rows on which the oracle has status 0 and is within 1e-13 of
    the truth -- long double arbitrates those at any bound, and the selection never looks at GPU output.  On several of them the
    one-pass recursion is more than BF_TARGET from the truth (asserted on the CPU from the numpy model): a guard that let them through
    would be caught.  Returns (X, rows, {row: truth})."""
    from burg_one_pass_model import adversarial_frames
    X = adversarial_frames(n, np.random.default_rng(11), count=120) * oracle.window("hanning_periodic", n)
    keep, truth = [], {}
    for f in range(X.shape[0]):
        if not np.all(np.isfinite(X[f])):
            continue
        st, co = oracle.lpc_burg(X[f], p)
        t = xt.burg(X[f], p) if st == 0 else None
        with np.errstate(all="ignore"):                       # an impulse: a row of zeros against a row of zeros
            if t is not None and xt.row_error(co, t) <= 1e-13:
                keep.append(f); truth[f] = t
    return np.ascontiguousarray(X), keep, truth
