"""The f64 kernels against a long-double truth (tests/extended_truth.py), not against 1e-6 of the oracle.

The oracle -- the reference's own f64 arithmetic -- is 1e-16 .. 1e-14 from the long-double result on well-conditioned input
(tests/test_extended_truth_math.py asserts E_O <= 1e-13 on every case used here).  Every other numerical GPU test grants a kernel 1e-6 of
the oracle: nine orders more than the arithmetic it replaces has.  Here, for a row A and its truth T,

    e(A) = max_j |A_j - T_j| / max_j |T_j|,      E_G = max over the case's rows of e(gpu row),   E_O = the same for the oracle's rows,

and with u = 2^-53:

  class I   (forms that claim rounding-level arithmetic: every autocorrelation kernel, every MFCC form, the direct Burg recursion, the sinc
            sums, the small operations):  E_G <= K * max(E_O, 4u), one K per family, K <= 16.  E_O is computed here from the oracle and
            the truth on the same rows, never from GPU output.  K was fixed from one recording run as the next power of two at or above
            twice the family's largest observed ratio, at least 2 (K_SET_FROM holds those ratios; the factor of two covers that a maximum
            over ~20 rows moves with the rows chosen).  An n-point FFT, a two-stage DFT or a 64-lane tree sum has a smaller worst-case
            bound than the reference's n-term sequential fold: a correct form sits at or below E_O, and one that needs more than 16 is a
            finding.
  class II  (the one-pass Burg, vbx_burg_fast.hpp, and its resampled lag form, which have a designed error budget): every row the fast path wrote is within
            BF_TARGET = 5e-7 of the TRUTH in the parity metric of conftest.rel_close; every row its guard handed to the direct recursion
            (identified by running the same frames under VBX_BURG_DIRECT=1 and comparing bits) meets class I.

            The direct Burg recursion at one frame per wavefront (G = 64: frames above 1024 samples or orders above 32) is class II as well: it
            carries the denominator from order to order, which amplifies rounding by (1 + mu^2) / (1 - mu^2) per order -- ~100 at the
            first order of 48 kHz speech.  The recording run measured E_G / E_O up to 123 on those shapes against 0.08 .. 0.24 on the
            directly summed ones; accuracy_cases.den_recursion_bound derives the bound d on the denominators' relative error from the
            truth's reflection coefficients.  Each of the p reflection coefficients then carries at most d, |mu_i| <= 1, and to first
            order a perturbed mu_i moves the row by its own size against the row's largest entry:
                e(row) <= K * max(e_O(row), 4u) + p * d(row)       (~4e-11 on speech rows, ~1e-13 on the noise row; observed: 2.4e-13).

What a caller of the library runs is held the same way (accuracy_cases.FUSED_CASES and the burg-resampled-* cases):
  * the MFCC columns of the fused frame loop, vbx_analyze_frames_* -- the kernel profiled as `analyze`, which computes pitch, LPC and MFCC
    together: class I in the mfcc family, one case per instance (launch-specialised f64 / PCM, generic, float32, the deferred tail in the
    LPC rows kernel and in mfcc_rows, the tail in the wavefront, every 3rd / 4th bin of a longer transform, the split and the fused 4096
    form, one interpolated instance per plan);
  * Burg on the resampled frame, find_formants at a resample_ratio, on every loader path of tests/test_gpu_analyze_ex.py::SHAPES, ratios
    whose inverse is no integer among them (the formant_extraction example's 10000 / 44100): the direct shapes class I in burg_direct (none
    of them is a G = 64 shape: vbx_burg_resampled_direct.hpp), the one-pass and dense-fallback shapes class II.
Their pitch, LPC and formant columns are not here: Brent (below), tests/test_gpu_lpc_exact.py, bit-equality with find_formants.

Which kernel ran is asserted from vbx_profile_names and the library's probes (vbx_internal_last_mfcc_form, last_burg_direct_count,
last_analyze_spec, last_spectral_split, last_autocorr_long_splits), as tests/test_gpu_layouts.py does.  The fused call has no probe for "bins interpolated": `analyze`
profiled, no MFCC kernel beside it and a frame that does not divide the transform leave launch_analyze no other form.
vbx_autocorrelate_f64 has no plan probe: the profile name autocorr_fft plus the frame length decide the transform (spectral_plan(),
restated in accuracy_cases.fft_transform), and the report test asserts that all four were reached.

The report (every case's E_G, E_O, ratio and probe; K and what it was set from) is kept as a file when VBX_TEST_REPORT_DIR names a
directory (as tests/test_gpu_layouts.py keeps its own); profiles/accuracy/report.json is the committed copy.

Not here, on purpose: the polynomial root finders (their error is the polynomial's conditioning), the tracker and the pitch path (discrete,
held bit for bit elsewhere), the Brent refinement (chaotic below its stopping step by design), the f32 entry points (tests/test_gpu_f32.py),
Levinson (tests/test_gpu_lpc_exact.py)."""
import json
import os

import numpy as np
import pytest

import accuracy_cases as ac
import extended_truth as xt
from conftest import rel_close

pytestmark = pytest.mark.gpu

U = xt.U
BF_TARGET = 5e-7                                             # vbx_burg_fast.hpp
K = {"autocorrelation": 4, "mfcc": 8, "burg_direct": 2, "sinc": 2, "small_ops": 4}
# family -> the largest E_G / max(E_O, 4u) of the recording runs and the case it came from; K = the next power of two at or above twice
# that, at least 2.  The second recording run (the fused frame loop's MFCC columns, Burg on the resampled frame) moved two of them:
#   mfcc 1.148 (mfcc-1200-goertzel) -> 2.793: the fused kernel's interpolated bins at 1600 samples in the 2048 plan.  M / n = 2.56 is just
#     inside the 32-tap class (mfcc_interp_taps, k_spectral.hip: tau = 0.305 against the class's edge at 0.298), where the taps' designed
#     cut, e^{-pi tau W} / (pi W / 2) = 1e-15 of the transform's largest bin, is at its largest; E_G there is 1.3e-15 against 4e-16 .. 5e-16 at
#     every other length.  The design's own figure, not a defect -- and by the rule above K goes from 4 to 8.
#   burg_direct 0.235 (burg-direct-512x12) -> 0.933: the direct recursion on the resampled view at order 20; K stays 2.
K_SET_FROM = {"autocorrelation": 1.041, "mfcc": 2.793, "burg_direct": 0.933, "sinc": 0.611, "small_ops": 1.008}
K_SET_FROM_CASE = {"autocorrelation": "autocorr-1281x300-tiles", "mfcc": "fused-mfcc-1600-interp", "burg_direct": "burg-resampled-1200-r1:4x20",
                   "sinc": "sinc-depth30", "small_ops": "dct-64"}
REPORT = {"cases": {}, "one_pass_rows": {}}


@pytest.fixture(scope="module")
def speech(vb):
    d = vb.synth_speech(ac.SPEECH_SAMPLES, sample_offset=ac.SPEECH_OFFSET)
    a = d.numpy()
    d.free()
    return a


def _note(name, family, e_g, e_o, **probe):
    ratio = e_g / max(e_o, 4 * U)
    REPORT["cases"][name] = dict(family=family, E_G=e_g, E_O=e_o, ratio=ratio, **probe)
    print(f"\naccuracy {name}: E_G {e_g:.3e}  E_O {e_o:.3e}  ratio {ratio:.3f}  (K {K.get(family)})  {probe}")
    return ratio


def _class_one(name, family, e_g, e_o, **probe):
    ratio = _note(name, family, e_g, e_o, **probe)
    assert e_g <= K[family] * max(e_o, 4 * U), (name, "E_G", e_g, "E_O", e_o, "ratio", ratio, "K", K[family])


def _call(ctx, case, X, monkeypatch):
    """One call of the case's entry point under its per-call switches; returns (rows, probes) and asserts the kernel that ran."""
    ctx.profile_reset()
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    try:
        if case.family == "autocorr":
            got = ctx.autocorrelate(X, case.p["lags"])
        elif case.family == "mfcc":
            got, st = ctx.mfcc(X, case.p["nc"], (case.p["lo"], case.p["hi"]), case.p["sr"])
            assert np.all(st == 0), (case, st)
        elif case.family == "burg_resampled":
            r = ctx.find_formants(X, ac.SR, case.p["order"], ac.EST0, resample_ratio=case.p["ratio"], want=("coeffs", "status"))
            got, st = r["coeffs"], r["status"]
            assert np.all(st == 0), (case, st)
        else:
            got, st = ctx.lpc_praat(X, case.p["order"])
            assert np.all(st == 0), (case, st)
    finally:
        for k in case.env:
            monkeypatch.delenv(k)
    names = set(ctx.profile_report())
    assert case.kernels <= names, (case, "expected kernels", sorted(case.kernels), "profiled", sorted(names))
    probe = {"kernels": sorted(names)}
    if case.family == "autocorr" and "autocorr_fft" in names:
        probe["fft_transform"] = ac.fft_transform(case.n)
    if "autocorr_long" in case.kernels:
        # into how many partial sums the launch cut each lag's sum: from the library, which reads it off the launch's own scratch size
        probe["long_splits"] = int(ctx.L.vbx_internal_last_autocorr_long_splits(ctx.ctx))
        assert probe["long_splits"] == case.p.get("splits", probe["long_splits"]) and probe["long_splits"] >= 1, (case, probe)
    if case.family == "mfcc":
        probe["mfcc_form"] = int(ctx.L.vbx_internal_last_mfcc_form(ctx.ctx))
        assert case.form is None or probe["mfcc_form"] == case.form, (case, probe)
    if case.family.startswith("burg"):
        probe["burg_direct_count"] = ctx.last_burg_direct_count()
        assert (probe["burg_direct_count"] >= 0) == (case.cls == 2), (case, probe)
    return got, probe


def _run(vb, pkg, case, X, monkeypatch):
    if not case.ctx_env:
        vb.profile(True)
        try:
            return _call(vb, case, X, monkeypatch)
        finally:
            vb.profile(False)
    for k, v in case.ctx_env.items():
        monkeypatch.setenv(k, v)
    own = pkg.VoxBox(0)
    for k in case.ctx_env:
        monkeypatch.delenv(k)
    try:
        own.profile(True)
        return _call(own, case, X, monkeypatch)
    finally:
        own.close()


def _direct_burg_rows(name, case, X, got, rows, e_o, truth, **probe):
    """Rows of the direct recursion: class I, or -- at the shapes whose kernel carries the denominator -- the derived class II bound."""
    e_g = {f: xt.row_error(got[f], truth[f]) for f in rows}
    p = case.p["order"]
    if not ac.den_recursion(ac.burg_len(case), p):           # (a resampled frame: the length and the samples Burg's kernel sees)
        return _class_one(name, "burg_direct", max(e_g.values()), max(e_o[f] for f in rows), rows=len(rows), **probe)
    bound = {f: K["burg_direct"] * max(e_o[f], 4 * U) + p * ac.den_recursion_bound(ac.burg_view(case, X[f]), p) for f in rows}
    _note(name, "burg_den_recursion", max(e_g.values()), max(e_o[f] for f in rows), rows=len(rows),
          derived_bound={int(f): bound[f] for f in rows}, E_G_rows={int(f): e_g[f] for f in rows}, **probe)
    for f in rows:
        assert e_g[f] <= bound[f], (name, f, "e", e_g[f], "bound", bound[f], "e_O", e_o[f])


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.cls == 1], ids=lambda c: c.id)
def test_class_one(vb, pkg, oracle, speech, monkeypatch, case):
    X = ac.frames(case, speech, oracle)
    got, probe = _run(vb, pkg, case, X, monkeypatch)
    keep, out, e_o, truth = ac.compared_rows(oracle, case, X)
    assert len(out) <= len(ac.rows(case)) // 8 and 0 in keep and case.F - 1 in keep, (case, out)
    if case.family in ("burg_direct", "burg_resampled"):
        if case.family == "burg_resampled":
            assert got.shape[1] == case.p["order"] and ac.burg_len(case) == case.p["m"] == int(vb.L.vbx_resampled_len(case.n, case.p["ratio"]))
        return _direct_burg_rows(case.id, case, X, got, keep, e_o, truth, **probe)
    e_g = max(xt.row_error(got[f], truth[f]) for f in keep)
    _class_one(case.id, ac.FAMILY_OF[case.family], e_g, max(e_o.values()), rows=len(keep), **probe)


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.cls == 2], ids=lambda c: c.id)
def test_one_pass_burg_against_the_truth(vb, pkg, oracle, speech, monkeypatch, case):
    """Class II.  The rows the one-pass form wrote: within BF_TARGET of the truth (until now: of the oracle).  The rows its guard sent to the
    direct recursion: class I.  The fast rows' E_G / E_O goes into the report: the header's "~1e-11 of the row's largest on speech" as a
    recorded number."""
    X = ac.frames(case, speech, oracle)
    fast, probe = _run(vb, pkg, case, X, monkeypatch)
    monkeypatch.setenv("VBX_BURG_DIRECT", "1")
    try:
        if case.family == "burg_resampled":
            r = vb.find_formants(X, ac.SR, case.p["order"], ac.EST0, resample_ratio=case.p["ratio"], want=("coeffs", "status"))
            direct, st = r["coeffs"], r["status"]
        else:
            direct, st = vb.lpc_praat(X, case.p["order"])
        assert vb.last_burg_direct_count() == -1 and np.all(st == 0)
    finally:
        monkeypatch.delenv("VBX_BURG_DIRECT")
    keep, out, e_o, truth = ac.compared_rows(oracle, case, X)
    assert len(out) <= len(ac.rows(case)) // 8 and 0 in keep and case.F - 1 in keep, (case, out)
    handed = [f for f in keep if np.array_equal(fast[f], direct[f])]
    wrote = [f for f in keep if f not in handed]
    assert wrote, (case, "the fast path wrote no compared row", handed, probe)
    ratios = {}
    for f in wrote:
        t = np.asarray(truth[f], dtype=np.float64)          # the bound is 5e-7: the truth rounded to f64 is exact enough
        assert np.all(rel_close(fast[f], t, BF_TARGET)), (case, f, fast[f], t)
        ratios[f] = xt.row_error(fast[f], truth[f]) / max(e_o[f], 4 * U)
    REPORT["one_pass_rows"][case.id] = {"rows_written_by_the_fast_path": len(wrote), "rows_handed_to_the_direct_recursion": len(handed),
                                       "E_G_over_E_O": {"min": min(ratios.values()), "median": float(np.median(list(ratios.values()))),
                                                        "max": max(ratios.values())},
                                       "E_G_max": max(xt.row_error(fast[f], truth[f]) for f in wrote), **probe}
    print(f"\naccuracy {case.id}: one-pass rows {REPORT['one_pass_rows'][case.id]}")
    if handed:
        _direct_burg_rows(case.id + "/handed-rows", case, X, fast, handed, e_o, truth)


def test_one_pass_guard_against_the_truth(vb, oracle, monkeypatch):
    """Class II where the guard has work to do (accuracy_cases.guard_case): of the rows long double can arbitrate, every one the fast path
    wrote is within BF_TARGET of the truth, and the guard handed some of them on.  (The rows it hands on are near-singular problems: the
    direct recursion's own rows are held by tests/test_gpu_burg_one_pass.py.)"""
    X, keep, truth = ac.guard_case(oracle)
    vb.profile(True)
    try:
        vb.profile_reset()
        fast, st = vb.lpc_praat(X, 12)
        sent = vb.last_burg_direct_count()
        assert {"burg_lags", "burg_recursion", "burg_direct_list"} <= set(vb.profile_report())
    finally:
        vb.profile(False)
    monkeypatch.setenv("VBX_BURG_DIRECT", "1")
    try:
        direct, sd = vb.lpc_praat(X, 12)
    finally:
        monkeypatch.delenv("VBX_BURG_DIRECT")
    assert np.array_equal(st, sd) and np.all(st[keep] == 0) and sent > 0
    wrote = [f for f in keep if not np.array_equal(fast[f], direct[f])]
    worst = 0.0
    for f in wrote:
        t = np.asarray(truth[f], dtype=np.float64)
        worst = max(worst, float(np.max(np.abs(fast[f] - t) / np.maximum(np.abs(t), 1e-6 * np.max(np.abs(t))))))
        assert np.all(rel_close(fast[f], t, BF_TARGET)), (f, fast[f], t)
    REPORT["one_pass_rows"]["guard-case-512x12"] = {"rows_compared": len(keep), "rows_written_by_the_fast_path": len(wrote),
                                                    "burg_direct_count": sent, "worst_parity_distance_from_the_truth": worst}
    print(f"\naccuracy guard case: {REPORT['one_pass_rows']['guard-case-512x12']}")
    assert 0 < len(wrote) < len(keep), (len(wrote), len(keep))


@pytest.fixture(scope="module")
def fused_stream(vb, speech):
    """the speech fixture's stream continued to the length the longest fused case needs (accuracy_cases.FUSED_SAMPLES)"""
    d = vb.synth_speech(ac.FUSED_SAMPLES, sample_offset=ac.SPEECH_OFFSET)
    a = d.numpy()
    d.free()
    assert np.array_equal(a[:speech.size], speech)
    return a


def _fused_call(ctx, pkg, case, up):
    """vbx_analyze_frames_f64 / _pcm16 / _ex_f32in on the case's stretch: (MFCC columns [F, nc], probes); asserts the instance that ran"""
    params = pkg.AnalysisParams.make(ac.SR, lpc_order=case.lpc_order, formant_order=12, mfcc=(case.p["nc"], case.p["lo"], case.p["hi"]))
    c0, w = params.columns()["mfcc"]
    assert w == case.p["nc"]
    kw = dict(frame_len=case.n, stride=case.hop, n_frames=case.F)
    ctx.profile_reset()
    if case.sample == "pcm16":
        rec, st = ctx.analyze_frames_pcm16(up, params, **kw)
    elif case.sample == "f32":
        rec, st = ctx.analyze_frames_ex_f32in(up, params, None, **kw)
    else:
        rec, st = ctx.analyze_frames(up, params, **kw)
    names = set(ctx.profile_report())
    probe = {"kernels": sorted(names), "analyze_spec": int(ctx.L.vbx_internal_last_analyze_spec(ctx.ctx)),
             "spectral_split": int(ctx.L.vbx_internal_last_spectral_split(ctx.ctx)), "bins_interpolated": case.interp}
    assert np.all(st == 0), (case, st)
    # MFCC joined the fused kernel: no MFCC kernel beside it (mfcc_rows is the deferred log10 + DCT, a lane per record: no transform),
    # and the samples were read as they are (no widening pass)
    assert "analyze" in names and not any(k.startswith("mfcc") and k != "mfcc_rows" for k in names), (case, probe)
    assert not {"pcm16", "f32_to_f64"} & names, (case, probe)
    assert probe["analyze_spec"] == case.spec and probe["spectral_split"] == case.split, (case, probe)
    assert ("mfcc_rows" in names) == case.mfcc_rows and ("lpc_rows" in names) == (case.lpc_order == 12), (case, probe)
    # bins interpolated <=> the frame does not divide the transform the call took (launch_analyze has no other MFCC form for such a frame)
    assert case.interp == ((2 * case.plan) % case.n != 0)
    return rec[:, c0:c0 + w], probe


@pytest.mark.parametrize("case", ac.FUSED_CASES, ids=lambda c: c.id)
def test_fused_mfcc(vb, pkg, oracle, fused_stream, monkeypatch, case):
    """The MFCC columns of the fused frame loop -- the kernel profiled as `analyze`, computing pitch, LPC and MFCC together -- against
    the truth: class I in the mfcc family, one case per instance (accuracy_cases.FUSED_CASES).  Until now these records were held to
    1e-6 of the oracle and to other kernels at 1e-11."""
    up, wide = ac.fused_audio(case, fused_stream)
    if case.sample == "pcm16":                               # the truth's input is what vbx_pcm16_to_f64 writes
        d = vb.pcm16_to_f64(up)
        dev_wide = d.numpy()
        d.free()
        assert np.array_equal(dev_wide, wide)
    if not case.ctx_env:
        vb.profile(True)
        try:
            got, probe = _fused_call(vb, pkg, case, up)
        finally:
            vb.profile(False)
    else:
        for k, v in case.ctx_env.items():
            monkeypatch.setenv(k, v)
        own = pkg.VoxBox(0)
        for k in case.ctx_env:
            monkeypatch.delenv(k)
        try:
            own.profile(True)
            got, probe = _fused_call(own, pkg, case, up)
        finally:
            own.close()
    X = ac.fused_frames(case, wide, oracle)
    keep, out, e_o, truth = ac.compared_rows(oracle, case, X)
    assert len(out) <= len(ac.rows(case)) // 8 and 0 in keep and case.F - 1 in keep, (case, out)
    e_g = max(xt.row_error(got[f], truth[f]) for f in keep)
    _class_one(case.id, "mfcc", e_g, max(e_o.values()), rows=len(keep), **probe)


@pytest.mark.parametrize("depth", [30, 1200])
def test_sinc_sums(vb, oracle, speech, depth):
    """vbx_interpolate_sinc_f64 at the 300 interior points of test_interpolate_sinc_points (its tolerance there: 1e-9); scale max |y|."""
    y, offset, nx, xs = ac.sinc_case(oracle, speech)
    got, st = vb.interpolate_sinc(y, offset, nx, xs, depth)
    t, o = [], []
    for i, x in enumerate(xs):
        s, v = xt.interpolate_sinc(y, offset, nx, x, depth)
        so, vo = oracle.interpolate_sinc(y, offset, nx, x, depth)
        assert s == so == st[i] == 0
        t.append(v); o.append(vo)
    t, scale = np.array(t, dtype=xt.LD), xt.LD(np.max(np.abs(y)))
    _class_one(f"sinc-depth{depth}", "sinc", float(np.max(np.abs(xt.ld(got) - t)) / scale), float(np.max(np.abs(xt.ld(o) - t)) / scale),
               points=int(xs.size))


def _rows_error(a, t):
    return max(xt.row_error(x, y) for x, y in zip(a, t))


def test_normalize(vb, oracle, speech):
    r = ac.small_inputs(speech)["normalize"]
    t = [xt.normalize(x) for x in r]
    _class_one("normalize-7x100", "small_ops", _rows_error(vb.normalize(r), t), _rows_error([oracle.normalize(x) for x in r], t))


@pytest.mark.parametrize("n", [13, 40, 64])
def test_dct(vb, oracle, speech, n):
    r = ac.small_inputs(speech)["dct"][n]
    t = [xt.dct(x) for x in r]
    _class_one(f"dct-{n}", "small_ops", _rows_error(vb.dct(r), t), _rows_error([oracle.dct(x) for x in r], t))


@pytest.mark.parametrize("n", [100, 1200, 4096])
def test_rms(vb, oracle, speech, n):
    r = ac.small_inputs(speech)["frames"][n]
    t = [xt.rms(x) for x in r]
    _class_one(f"rms-{n}", "small_ops", _rows_error(vb.rms(r), t), _rows_error([oracle.rms(x) for x in r], t))


@pytest.mark.parametrize("n", [100, 1200, 4096])
def test_preemphasis(vb, oracle, speech, n):
    r = ac.small_inputs(speech)["frames"][n]
    t = xt.preemphasis(r, 0.1)
    _class_one(f"preemphasis-{n}", "small_ops", _rows_error(vb.preemphasis(r, 0.1), t), _rows_error([oracle.preemphasis(x, 0.1) for x in r], t))


def test_to_resonance(vb, oracle, speech):
    roots = ac.small_inputs(speech)["roots"]
    res, cnt = vb.to_resonance(roots, ac.SR)
    e_g = e_o = 0.0
    for f in range(roots.shape[0]):
        t, o = xt.to_resonance(roots[f], ac.SR), oracle.to_resonance(roots[f], ac.SR)
        assert cnt[f] == t.shape[0] == o.shape[0] and cnt[f] > 0
        e_g = max(e_g, xt.row_error(res[f, :cnt[f]].reshape(-1), t.reshape(-1)))
        e_o = max(e_o, xt.row_error(o.reshape(-1), t.reshape(-1)))
    _class_one("to_resonance-50x12", "small_ops", e_g, e_o)


def test_zz_accuracy_report():
    """Runs last in this file: all four FFT plans were reached, every class I family has K <= 16, and the report is written."""
    cases = REPORT["cases"]
    if all(c.id in cases for c in ac.CASES if c.cls == 1):   # (a selection of this file's tests: no statement about the rest)
        assert {c.get("fft_transform") for c in cases.values()} >= {1024, 1200, 2048, 4096}
    assert all(2 <= k <= 16 for k in K.values())
    fam = {}
    for c in cases.values():
        fam[c["family"]] = max(fam.get(c["family"], 0.0), c["ratio"])
    REPORT["families"] = {f: {"largest_ratio_this_run": fam.get(f), "K": K[f], "K_set_from_ratio": K_SET_FROM.get(f),
                              "K_set_from_case": K_SET_FROM_CASE.get(f)} for f in K}
    for f in K:                                              # K follows its own rule: the next power of two at or above twice the recorded ratio
        assert K[f] == max(2, 1 << int(np.ceil(np.log2(2 * K_SET_FROM[f])))), (f, K[f], K_SET_FROM[f])
    REPORT["metric"] = "E = max over rows of max_j |A_j - T_j| / max_j |T_j|, T in long double; ratio = E_G / max(E_O, 4 * 2^-53)"
    print("\naccuracy families:", json.dumps(REPORT["families"]))
    out = os.environ.get("VBX_TEST_REPORT_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "accuracy_report.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)
