"""The cases of the accuracy tests: tests/test_extended_truth_math.py (CPU: is the truth good enough, are the inputs well conditioned) and
tests/test_gpu_accuracy.py (GPU: the kernels against the truth) run THE SAME list on the same rows.

Frames: Hanning-windowed synthetic speech (the voiced glide of the stream the other GPU tests use) and, as the last row of every batch, one
rectangular noise frame: x[0] != 0 there, so the seed of the reference's autocorrelation fold counts.  The MFCC frames are scaled by 40,
as tests/test_gpu_parity.py scales them: every filter's energy is then well above the log10 clamp.

Batch sizes: one frame more than the kernel's frames per block, so the last wavefront (or block) is partial: 17 for the few-lag kernel and
the one-pass Burg (9 at frames of up to 512 samples), 64 / G + 1 for the direct Burg; the kernels that take one frame per block get 6 frames,
3 from 2048 samples up.  Truth is computed for at most 12 rows of a batch (3 from 2048 samples up), the first and the last always.

Two groups hold what a caller of the library runs: find_formants at a resample_ratio on every path of the resampled loaders (appended to
CASES: unwindowed frames, 17 per batch) and the MFCC columns of the fused frame loop (FUSED_CASES, a list and an input of its own)."""
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
    _ac(4097, 40, "long", splits=5),
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


def _rs(n, ratio, tag, p, m, kernels, cls):
    """find_formants at a resample_ratio, one case per loader path of tests/test_gpu_analyze_ex.py::SHAPES (m: the resampled length)"""
    return Case(f"burg-resampled-{n}-{tag}x{p}", "burg_resampled", n, 17, kernels=kernels, rect=True, cls=cls, order=p, ratio=ratio, m=m)


_DIRECT, _ONE_PASS, _DENSE = {"burg_resampled"}, {"burg_lags_resampled", "burg_recursion"}, {"resample", "burg_lags", "burg_recursion"}
# appended, never inserted: frames() takes a case's input offset from its index in CASES
CASES += [
    # -- the direct recursion on the resampled view: 4 frames per wavefront (the formant_extraction example's own shape and ratio), m below
    #    the one-pass forms' 256, an odd m that ends inside a lane, orders off the one-pass list (order 20: 32 lanes per frame)
    _rs(500, 10000.0 / 44100.0, "r10000:44100", 13, 114, _DIRECT, 1), _rs(1200, 10000.0 / 48000.0, "r10000:48000", 12, 250, _DIRECT, 1),
    _rs(1103, 10000.0 / 44100.0, "r10000:44100", 13, 251, _DIRECT, 1), _rs(1200, 0.25, "r1:4", 5, 300, _DIRECT, 1),
    _rs(1200, 0.25, "r1:4", 20, 300, _DIRECT, 1),
    # -- the one-pass lag kernel on the resampled view at 16 and 20 samples per lane, and upsampling (the last outputs read past the frame)
    _rs(2048, 0.5, "r1:2", 16, 1024, _ONE_PASS, 2), _rs(2400, 0.5, "r1:2", 12, 1200, _ONE_PASS, 2), _rs(200, 1.5, "r3:2", 8, 300, _ONE_PASS, 2),
    # -- the dense fallback: resampled into a batch, then the plain one-pass form (m = 2048; a source frame beyond VBX_MAX_FRAME_LEN)
    _rs(4096, 0.5, "r1:2", 12, 2048, _DENSE, 2), _rs(5000, 0.2, "r1:5", 12, 1000, _DENSE, 2),
]


def long_splits(F, n, lags):
    """autocorr_long_splits() of k_long.hip, restated to CHOOSE the cases' frame counts: into how many partial sums a launch of F long frames
    cuts each lag's sum -- enough for 1280 workgroups, at most one per 1024-sample chunk of the frame, at most 64.  What a case claims is
    held to the library on the GPU: tests/test_gpu_accuracy.py asserts vbx_internal_last_autocorr_long_splits == the case's `splits`."""
    groups, chunks = -(-lags // 1280), -(-n // 1024)
    return max(1, min(-(-1280 // (F * groups)), chunks, 64))


def _acl(n, lags, F, hop, splits):
    assert long_splits(F, n, lags) == splits
    return Case(f"autocorr-{n}x{lags}-long-{F}-frames-{splits}-splits", "autocorr", n, F, kernels={"autocorr_long"}, lags=lags, hop=hop, splits=splits)


# -- the long-frame autocorrelation at every form of its summation split, which follows the launch's frame count: one sum per lag (what every
#    large call runs), three partial sums, one per chunk of a 4097-sample frame alone, and the cap of 64 at 65,537 samples.  (autocorr-4097x40-long
#    above: 3 frames, 5 splits.)  These batches are too large for frames 997 samples apart: a hop of their own.
CASES += [_acl(4097, 40, 1280, 3, 1), _acl(4097, 40, 500, 101, 3), _acl(4097, 40, 1, 997, 5), _acl(65537, 13, 1, 997, 64)]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

FAMILY_OF = {"autocorr": "autocorrelation", "mfcc": "mfcc", "burg_direct": "burg_direct", "burg_fast": "burg_direct"}
EST0 = np.array([[320.0, 1.0], [1440.0, 1.0], [2760.0, 1.0], [3200.0, 1.0]])


# ---- the fused frame loop's MFCC columns (vbx_analyze_frames_*: the kernel profiled as `analyze`) ----------------------------------------
# One case per instance of the fused kernel that computes MFCC next to pitch and LPC.  Input: one contiguous stretch of the stream,
# (F - 1) hop + n samples from the speech fixture's first sample, times 40 (the MFCC scaling above); F = 67 frames -- more than one
# wavefront of frames, so they are dealt across the XCDs.  The two longest cases need 139,264 samples: 43,264 more than the fixture's
# two voiced seconds, so their stretch runs on into the stream's unvoiced second (their last compared row is noise at 0.05 * 40).
FUSED_F = 67
FUSED_SAMPLES = (FUSED_F - 1) * 2048 + 4096
PCM_GAIN = 3180.0                                            # 16-bit units per unit of the scaled stretch: its peak, 10.29, lands at 32,720


class FusedCase:
    """n / hop; sample: f64, pcm16 or f32; ctx_env: the switches a context of its own is created under; spec / split / mfcc_rows / interp:
    what vbx_internal_last_analyze_spec, vbx_internal_last_spectral_split and vbx_profile_names must say, and whether the frame's bins lie
    between the transform's (2 * spectral_plan_nc(plan) % n != 0: the fused call has no probe for that)."""

    def __init__(self, tag, n, hop, plan, spec=0, split=0, mfcc_rows=False, sample="f64", ctx_env=None, nc=13, lpc_order=12):
        self.id, self.n, self.hop, self.plan, self.F = f"fused-mfcc-{n}-{tag}", n, hop, plan, FUSED_F
        self.spec, self.split, self.mfcc_rows, self.sample, self.ctx_env = spec, split, mfcc_rows, sample, ctx_env or {}
        self.family, self.lpc_order = "mfcc", lpc_order
        self.p = dict(nc=nc, lo=100.0, hi=8000.0, sr=SR)
        self.interp = (2 * plan) % n != 0

    def __repr__(self):
        return self.id


FUSED_CASES = [
    # -- 1200 / 480, the headline shape: the launch-specialised instance with the tail deferred into the LPC rows kernel; without LPC
    #    (mfcc_rows finishes the rows); 20 coefficients (generic instance, tail in the wavefront); the two switches; PCM; float32
    FusedCase("default", 1200, 480, 1200, spec=1), FusedCase("no-lpc", 1200, 480, 1200, spec=1, mfcc_rows=True, lpc_order=0),
    FusedCase("20-coefficients", 1200, 480, 1200, nc=20), FusedCase("generic", 1200, 480, 1200, ctx_env={"VBX_SPECTRAL_SPEC": "0"}),
    FusedCase("tail-in-the-wavefront", 1200, 480, 1200, ctx_env={"VBX_MFCC_DEFER": "0"}),
    FusedCase("pcm16", 1200, 480, 1200, spec=2, sample="pcm16"), FusedCase("float32", 1200, 480, 1200, sample="f32"),
    # -- zero-padded frames in the 1200 plan: every 3rd and every 4th bin of its 2400 points
    FusedCase("every-3rd-bin", 800, 320, 1200), FusedCase("every-4th-bin", 600, 240, 1200),
    # -- the power-of-two plans (512: every 4th bin of the 1024 plan's 2048 points); 4096 as two kernels and as one
    FusedCase("pow2", 1024, 512, 1024), FusedCase("every-4th-bin", 512, 256, 1024), FusedCase("pow2", 2048, 1024, 2048),
    FusedCase("split", 4096, 2048, 4096, split=1), FusedCase("one-kernel", 4096, 2048, 4096, ctx_env={"VBX_POW2_SPLIT": "0"}),
    # -- bins interpolated from the transform's: one instance per plan, and an odd length
    FusedCase("interp", 700, 350, 1024), FusedCase("interp", 1103, 441, 1200), FusedCase("interp-odd", 1199, 480, 1200),
    FusedCase("interp", 1600, 640, 2048), FusedCase("interp", 3000, 1200, 4096, split=1), FusedCase("interp", 4000, 2000, 4096, split=1),
]
assert len({c.id for c in FUSED_CASES}) == len(FUSED_CASES) and all(c.plan == fft_transform(c.n) or (2 * 1200) % c.n == 0 for c in FUSED_CASES)
assert [c.id for c in FUSED_CASES if c.interp] == [f"fused-mfcc-{n}-interp" + ("-odd" if n == 1199 else "") for n in (700, 1103, 1199, 1600, 3000, 4000)]


def fused_audio(case, stream):
    """(what is uploaded, the f64 samples the kernel's arithmetic starts from) for a stream of at least FUSED_SAMPLES samples.  PCM: the
    widened sample is int16 / 32767 (vbx_pcm16_to_f64: one correctly rounded division); float32: the float cast to f64, exactly."""
    a = stream[:(case.F - 1) * case.hop + case.n] * 40.0
    if case.sample == "pcm16":
        pcm = np.rint(a * PCM_GAIN).astype(np.int16)
        return pcm, pcm.astype(np.float64) / 32767.0
    if case.sample == "f32":
        f = a.astype(np.float32)
        return f, f.astype(np.float64)
    return a, a


def fused_frames(case, wide, oracle):
    """[F, n]: the windowed frames of the compared rows (zero rows elsewhere), the window product in f64 as the oracle takes it"""
    X = np.zeros((case.F, case.n))
    w = oracle.window("hanning", case.n)
    for f in rows(case):
        X[f] = wide[f * case.hop:f * case.hop + case.n] * w
    return X


def host_speech():
    """the same stream from the host statement of the generator (within 1e-9 of the device's): what the CPU test conditions on"""
    import importlib
    import __graft_entry__ as g
    g.load_package()
    return importlib.import_module(g.PKG_NAME + ".synth").synth_speech(SPEECH_SAMPLES, sample_offset=SPEECH_OFFSET)


def frames(case, speech, oracle):
    k = CASES.index(case)
    base, hop = 1000 + 3001 * (k % 8), case.p.get("hop", 997)
    assert base + (case.F - 1) * hop + case.n <= speech.size, case
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


def burg_view(case, x):
    """what Burg's recursion runs on: the frame itself, or -- find_formants at a resample_ratio -- its resampled view under the periodic
    Hanning window, in long double"""
    if case.family != "burg_resampled":
        return x
    x = xt.resample_linear(x, case.p["ratio"])
    return x * xt.periodic_hanning(x.size)


def burg_len(case):
    """the length Burg's kernels see (what chooses the direct recursion's lane group)"""
    return int(np.ceil(case.p["ratio"] * case.n)) if case.family == "burg_resampled" else case.n


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
            t = xt.burg(burg_view(case, X[f]), case.p["order"], reverse)
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
