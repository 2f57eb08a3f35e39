"""The fused frame loop (vbx_analyze_frames_f64 / _pcm16) away from the one pitch setting the rest of the suite calls it with
(threshold 0.2, fmin 75 Hz, fmax 600 Hz), on a real MI355X.

The three pitch parameters steer the part of analyze_kernel that is edited most: how much of the lag curve is kept
(pitch_curve_entries / pitch_curve_reach = 2 ceil(sr / fmin) + 16, also the split form's scratch row), how many peaks pass the
frequency filter (one lane or four per candidate in the bounds), what the exact top-1 pruning may skip (every bound below the
unvoiced candidate's strength, i.e. the threshold), and which frames go to the direct-sum fallback (a peak on fmin / fmax), whose
write lands in a record row.  vbx_pitch_f64 is held to the oracle at many settings, but it is another set of template instances:
each fused instance (LPC, MFCC, pow2 / split / interpolated MFCC) has its own registers, LDS layout and spills.

  1. the sweep: 13 shapes (one per kernel form) x 11 settings x 48 frames that span the glide and the noise-only second, the
     whole record against the CPU oracle (tests/analyze_reference.py), against the same call at the default setting (pitch
     parameters touch no other column: bit for bit) and against vbx_pitch_f64(kmax = 1);
  2. a sub-grid again for the other instances (pitch only, no MFCC, no LPC, LPC order 10);
  3. split = fused and cut curve = whole curve for the fused RECORD at fmin from 0 to 400 Hz, bit for bit;
  4. degenerate frames (noise, tones, impulses, silence, 1e-150 .. 1e120, NaN, Inf) among ordinary ones in one batch;
  5. the PCM form and non-finite / negative pitch parameters.

Tolerances are BASELINE's (1e-4 relative Hz, 1e-4 strength, 1e-6 MFCC / LPC), the top-candidate rule and its caps are those of
tests/test_gpu_parity.py::_check_pitch: per case bad == 0, vuv_outside == 0, swap <= 1; over the file swaps <= 0.2 % of the frames.
tests/test_analyze_reference.py shows on the CPU that the inputs themselves never need the swap allowance.  No frame is left out of
a comparison for any reason but an oracle status that is not OK, and then the status (and the zero pair) is what is compared."""
import json
import os

import numpy as np
import pytest

import analyze_reference as ar
from conftest import rel_close

pytestmark = pytest.mark.gpu

P = 12
F = ar.SWEEP_FRAMES
REPORT = {"sweep": {}, "instances": [], "forms": [], "degenerate": [], "pcm16": [], "parameters": []}

# the instances launch_analyze picks by what else the record holds
FULL = dict(lpc_order=P, formant_order=P, mfcc=True)
VARIANTS = {"pitch only": dict(lpc_order=0, formant_order=0, mfcc=False),
            "LPC, no MFCC": dict(lpc_order=P, formant_order=P, mfcc=False),
            "MFCC, no LPC": dict(lpc_order=0, formant_order=P, mfcc=True),
            "LPC order 10 beside the fused kernel": dict(lpc_order=10, formant_order=P, mfcc=True)}
SUB_SHAPES = [(1200, 480, 48000.0), (1024, 512, 48000.0), (2048, 1024, 48000.0), (4096, 2048, 48000.0)]
SUB_SETTINGS = ("0.2/120/200", "1.5/75/600", "0.2/100/20000", "0.2/400/sr")


def _key(shape):
    return "%d/%d@%g" % shape


def _id(shape):
    return "%d-%d-%g" % shape


class _Bank:
    """Per shape: the sweep's signal on the device and on the host (the same samples on both sides), and the oracle's answers,
    computed once (pitch per setting; formants, MFCC and LPC do not depend on the pitch setting)."""

    def __init__(self, vb, pkg, oracle):
        self.vb, self.pkg, self.oracle, self.items = vb, pkg, oracle, {}
        self.est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])

    def get(self, shape):
        if shape not in self.items:
            n, _, sr = shape
            ns, off = ar.sweep_samples(n, sr)
            d = self.vb.synth_speech(ns, sample_offset=off, sample_rate=sr)
            self.items[shape] = dict(d=d, x=d.numpy(), stride=ar.sweep_stride(n, sr), pitch={}, other=None)
        return self.items[shape]

    def params(self, shape, pitch, lpc_order=P, formant_order=P, mfcc=True):
        return self.pkg.AnalysisParams.make(shape[2], pitch=pitch, lpc_order=lpc_order, formant_order=formant_order, est_init=self.est0,
                                            mfcc=ar.mfcc_band(shape[2]) if mfcc else None)

    def oracle_pitch(self, shape, pitch):
        it = self.get(shape)
        if pitch not in it["pitch"]:
            _, st, top2, cnt = ar.oracle_records(self.oracle, it["x"], shape[0], it["stride"], range(F), shape[2], pitch, 0, 0, None, None, None)
            it["pitch"][pitch] = (st[0], top2, cnt)
        return it["pitch"][pitch]

    def oracle_other(self, shape):
        """Formant and MFCC columns of the 48 frames as one segment: (records, status), formants in columns 2..10, MFCC in 10..23.
        (LPC is held to vbx_autocorr_lpc_f64's rows: under the default exact-row policy the oracle's own f64 Levinson rows are not
        the target on ill-conditioned frames, tests/test_gpu_lpc_exact.py owns that.)"""
        it = self.get(shape)
        if it["other"] is None:
            rec, st, _, _ = ar.oracle_records(self.oracle, it["x"], shape[0], it["stride"], range(F), shape[2], None, 0, P, self.est0,
                                              ar.mfcc_band(shape[2]), {0})
            it["other"] = (rec, st)
        return it["other"]

    def close(self):
        for it in self.items.values():
            it["d"].free()
        self.items = {}


@pytest.fixture(scope="module")
def bank(vb, pkg, oracle):
    b = _Bank(vb, pkg, oracle)
    yield b
    b.close()


def _judge_pitch(pairs, st_row, ost, top2, cnt):
    """A pitch column against the oracle: (counters, problems).  Status exact on every frame; where the oracle's status is not OK
    the pair is 0.0, 0.0 (what _check_pitch demands of vbx_pitch_f64); every other frame goes through classify_top."""
    c = dict(frames=len(ost), compared=0, ok=0, swap=0, vuv_outside=0, bad=0, voiced=0, status_not_ok=0)
    problems = []
    if not np.array_equal(st_row, ost):
        problems.append(("pitch status", np.flatnonzero(st_row != ost)[:5].tolist(), st_row.tolist(), ost.tolist()))
    for t in range(len(ost)):
        if ost[t] != 0:
            c["status_not_ok"] += 1
            if not (pairs[t, 0] == 0.0 and pairs[t, 1] == 0.0):
                problems.append(("pair of a frame whose status is not OK", t, pairs[t].tolist()))
            continue
        if np.isnan(top2[t, 0, 1]):                   # a NaN threshold on a frame with no other candidate: the same pair, NaN for NaN
            v = "ok" if np.array_equal(pairs[t], top2[t, 0], equal_nan=True) else "bad"
        else:
            v = ar.classify_top(pairs[t], top2[t], cnt[t])
        c["compared"] += 1
        c[v] += 1
        c["voiced"] += int(pairs[t, 0] > 0.0)
        if v in ("bad", "vuv_outside"):
            problems.append((v, t, pairs[t].tolist(), top2[t].tolist(), int(cnt[t])))
    if c["swap"] > 1:
        problems.append(("more than one tie swap in a case", c["swap"]))
    return c, problems


def _check_other_columns(bank, shape, variant, rec, st):
    """Formant, MFCC and LPC columns of a default-setting call against the oracle / vbx_autocorr_lpc_f64, as
    test_analyze_frames_matches_the_oracle_and_the_separate_entry_points does."""
    vb, pkg = bank.vb, bank.pkg
    n, _, sr = shape
    it = bank.get(shape)
    cols = bank.params(shape, ar.DEFAULT_PITCH, **variant).columns()
    orec, ost = bank.oracle_other(shape)
    problems = []
    if variant["formant_order"]:
        c0 = cols["formants"][0]
        if not np.array_equal(st[1], ost[1]):
            problems.append(("formant status", st[1].tolist(), ost[1].tolist()))
        ok = ost[1] == 0
        got, exp = rec[ok, c0:c0 + 8:2], orec[ok, 2:10:2]
        if not np.all(np.abs(got - exp) <= 1e-4 * np.abs(exp)):
            problems.append(("formant Hz", float(np.max(np.abs(got - exp) / np.abs(exp)))))
    elif st[1].any():
        problems.append(("formant status of a record without formants", st[1].tolist()))
    if variant["mfcc"]:
        c0 = cols["mfcc"][0]
        assert not ost[2].any() and np.all(np.isfinite(orec[:, 10:23])), "the band was chosen so that the oracle's MFCC is OK and finite"
        if st[2].any():
            problems.append(("MFCC status", st[2].tolist()))
        for t in range(F):
            if not np.all(rel_close(rec[t, c0:c0 + 13], orec[t, 10:23], 1e-6)):
                problems.append(("MFCC", t, float(np.abs(rec[t, c0:c0 + 13] - orec[t, 10:23]).max())))
    elif st[2].any():
        problems.append(("MFCC status of a record without MFCC", st[2].tolist()))
    if variant["lpc_order"]:
        order = variant["lpc_order"]
        c0 = cols["lpc"][0]
        han = vb.window(pkg.WINDOW_HANNING, n)
        _, a = vb.autocorr_lpc(it["d"], order, frame_len=n, stride=it["stride"], n_frames=F, window=han)
        if not np.all(rel_close(rec[:, c0:c0 + order + 1], a)):
            problems.append(("LPC against vbx_autocorr_lpc_f64", float(np.abs(rec[:, c0:c0 + order + 1] - a).max())))
    return problems


def _check_case(bank, shape, pitch, variant, base):
    """One (shape, setting, instance): the record against the oracle, against the default-setting call `base` = (rec, st), and
    against vbx_pitch_f64(kmax = 1).  Returns (counters, problems)."""
    vb, pkg = bank.vb, bank.pkg
    n, _, sr = shape
    it = bank.get(shape)
    rec, st = vb.analyze_frames(it["d"], bank.params(shape, pitch, **variant), frame_len=n, stride=it["stride"], n_frames=F)
    c, problems = _judge_pitch(rec[:, 0:2], st[0], *bank.oracle_pitch(shape, pitch))
    # pitch parameters touch nothing else (an odd record is padded to an even row; the pad is never written)
    rec0, st0 = base
    width = sum(w for _, w in bank.params(shape, pitch, **variant).columns().values())
    assert rec.shape == (F, width + (width & 1))
    a, b = rec[:, 2:width].view(np.int64), rec0[:, 2:width].view(np.int64)
    if not (np.array_equal(a, b) and np.array_equal(st[1:], st0[1:])):
        problems.append(("columns other than pitch differ from the default setting's", np.flatnonzero(np.any(a != b, axis=1))[:8].tolist(),
                         (2 + np.flatnonzero(np.any(a != b, axis=0)))[:8].tolist()))
    # the stand-alone entry point, same window, shape and setting
    han = vb.window(pkg.WINDOW_HANNING, n)
    cand, _, pst = vb.pitch(it["d"], sr, pitch[0], pitch[1], pitch[2], kmax=1, frame_len=n, stride=it["stride"], n_frames=F, window=han)
    cand = cand[:, 0, :]
    if not np.array_equal(st[0], pst):
        problems.append(("status differs from vbx_pitch_f64's", st[0].tolist(), pst.tolist()))
    if not np.array_equal(rec[:, 0] == 0.0, cand[:, 0] == 0.0):
        problems.append(("voiced / unvoiced decision differs from vbx_pitch_f64's", np.flatnonzero((rec[:, 0] == 0.0) != (cand[:, 0] == 0.0)).tolist()))
    if not (np.all(np.abs(rec[:, 0] - cand[:, 0]) <= 1e-4 * np.abs(cand[:, 0])) and np.all(np.abs(rec[:, 1] - cand[:, 1]) <= 1e-4)):
        problems.append(("values differ from vbx_pitch_f64's", float(np.abs(rec[:, 0] - cand[:, 0]).max()), float(np.abs(rec[:, 1] - cand[:, 1]).max())))
    c["not_bitwise_vs_pitch_f64"] = int(np.count_nonzero(np.any(rec[:, 0:2].view(np.int64) != cand.view(np.int64), axis=1)))
    return c, problems


@pytest.mark.parametrize("shape", ar.SHAPES, ids=_id)
def test_fused_record_across_pitch_settings(vb, pkg, oracle, bank, shape):
    """Every setting of the sweep at one shape, the full record (LPC 12, formants 12, 13 MFCCs): see the module's docstring."""
    n, _, sr = shape
    it = bank.get(shape)
    base = vb.analyze_frames(it["d"], bank.params(shape, ar.DEFAULT_PITCH), frame_len=n, stride=it["stride"], n_frames=F)
    assert base[0].shape == (F, 36) and base[1].shape == (3, F)
    failures = [("default setting", p) for p in _check_other_columns(bank, shape, FULL, *base)]
    out = REPORT["sweep"].setdefault(_key(shape), {})
    for name, pitch in zip(ar.SETTING_NAMES, ar.settings(n, sr)):
        c, problems = _check_case(bank, shape, pitch, FULL, base)
        out[name] = c
        print(_key(shape), name, c)
        failures += [(name, p) for p in problems]
    assert not failures, failures[:6]


@pytest.mark.parametrize("variant", list(VARIANTS), ids=lambda v: v.replace(" ", "_").replace(",", ""))
@pytest.mark.parametrize("shape", SUB_SHAPES, ids=_id)
def test_other_instances_across_pitch_settings(vb, pkg, oracle, bank, shape, variant):
    """The instances launch_analyze picks when the record holds less (or an LPC order the register Levinson is not built for):
    the same checks at the four settings that cut the band, prune everything, keep the most candidates and keep the shortest curve."""
    n, _, sr = shape
    it = bank.get(shape)
    v = VARIANTS[variant]
    base = vb.analyze_frames(it["d"], bank.params(shape, ar.DEFAULT_PITCH, **v), frame_len=n, stride=it["stride"], n_frames=F)
    failures = [("default setting", p) for p in _check_other_columns(bank, shape, v, *base)]
    for name, pitch in zip(ar.SETTING_NAMES, ar.settings(n, sr)):
        if name not in SUB_SETTINGS:
            continue
        c, problems = _check_case(bank, shape, pitch, v, base)
        REPORT["instances"].append(dict(shape=_key(shape), instance=variant, setting=name, **c))
        failures += [(name, p) for p in problems]
    assert not failures, failures[:6]


# ---- kernel forms that must agree bit for bit, away from 75 Hz ---------------------------------------------------------------

@pytest.mark.parametrize("n,hop", [(2048, 1024), (4096, 2048), (3000, 1200), (2205, 882)])
def test_fused_record_split_and_cut_forms_away_from_75_hz(pkg, monkeypatch, n, hop):
    """The 4096-point plan as two kernels (VBX_POW2_SPLIT) and the cut lag curve (VBX_PITCH_CURVE_CUT) are compared elsewhere at
    fmin = 75 Hz, or through vbx_pitch_f64 only.  Here the fused RECORD: fmin from none to 400 Hz (the scratch row and the kept curve
    from everything down to 2 * 120 + 16 lags), no ceiling, thresholds 0.2 and 0: split = one kernel and cut = whole curve, every
    column and status bit for bit.  2,000 frames of the synthetic recording per case and five odd frames (noise, 76 Hz, 30 Hz, square,
    DC + noise).  One context per switch value, created and closed in turn."""
    sr, frames = 48000.0, 2000
    rng = np.random.default_rng(n)
    t = np.arange(n) / sr
    odd = np.array([rng.standard_normal(n), np.sin(2 * np.pi * 76.0 * t), np.sin(2 * np.pi * 30.0 * t), np.sign(np.sin(2 * np.pi * 80 * t)),
                    0.5 + 0.01 * rng.standard_normal(n)])
    est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    cases = [(thr, fmin) for thr in (0.2, 0.0) for fmin in (ar.pitch_edge(n, sr), 20.0, 120.0, 400.0, 0.0)]
    got = {}
    for form, var, val in (("default", None, None), ("split", "VBX_POW2_SPLIT", "1"), ("one kernel", "VBX_POW2_SPLIT", "0"),
                           ("whole curve", "VBX_PITCH_CURVE_CUT", "0")):
        if var:
            monkeypatch.setenv(var, val)
        ctx = pkg.VoxBox(0)
        if var:
            monkeypatch.delenv(var)
        try:
            audio = ctx.synth_speech((frames - 1) * hop + n, sample_offset=2 * 48000)
            res = []
            for thr, fmin in cases:
                params = pkg.AnalysisParams.make(sr, pitch=(thr, fmin, 20000.0), lpc_order=P, formant_order=P, est_init=est0, mfcc=(13, 100.0, 8000.0))
                rec, st = ctx.analyze_frames(audio, params, frame_len=n, stride=hop, n_frames=frames)
                split = int(ctx.L.vbx_internal_last_spectral_split(ctx.ctx))
                orec, ost = ctx.analyze_frames(odd, params)
                res.append((rec.copy(), st.copy(), orec.copy(), ost.copy(), split))
            got[form] = res
            audio.free()
        finally:
            ctx.close()
    for a_name, b_name in (("split", "one kernel"), ("default", "whole curve")):
        for (thr, fmin), a, b in zip(cases, got[a_name], got[b_name]):
            for what, x, y in zip(("records", "status", "records of the odd frames", "status of the odd frames"), a[:4], b[:4]):
                same = _same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)
                assert same, (a_name, b_name, thr, fmin, what, np.argwhere(x != y)[:8].tolist())
    assert all(r[4] == 0 for r in got["one kernel"])
    if n > 2048:
        assert any(r[4] == 1 for r in got["split"]), "the split form never ran"
    voiced = [int(np.count_nonzero(r[0][:, 0])) for r in got["default"]]
    assert min(voiced) > 50, voiced                                            # voiced frames in every case
    REPORT["forms"].append(dict(shape="%d/%d" % (n, hop), cases=len(cases), frames_per_case=frames + 5,
                                split_ran=[r[4] for r in got["split"]], voiced=voiced))


# ---- degenerate frames through the fused call ---------------------------------------------------------------------------------

def _speech_rows(vb, n, sr, rows, hop=997):
    d = vb.synth_speech((rows - 1) * hop + n, sample_offset=int(2 * sr), sample_rate=sr)
    x = d.numpy()
    d.free()
    return np.array([x[i * hop:i * hop + n] for i in range(rows)])


def _same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("n", [1200, 1024, 4096, 5000])
def test_degenerate_frames_among_ordinary_ones(vb, pkg, oracle, n):
    """Noise, tones, a clipped tone, squares, a chirp, five impulses, DC + noise, silence, 1e-150 .. 1e120 amplitudes and one NaN / one
    Inf sample (17 classes, six frames each) shuffled among 98 ordinary frames, every frame its own segment, through ONE fused call:
    the three parts share a transform and a record row, and a bad frame's neighbours sit in the same workgroup's batch.  Statuses of
    all three parts exact against the oracle, pitch through classify_top, MFCC within 1e-6, formant Hz within 1e-4 where the
    oracle's own answer is stable (the probe of test_mfcc_and_formants_odd_signals); frames were deferred to the direct-sum fallback
    inside the fused call (not at 5,000 samples: no FFT path to defer from) and their records are complete; the ordinary frames'
    rows are bit for bit those of the same call with the degenerate frames replaced by ordinary ones."""
    sr = 48000.0
    total = 98 + 6 * len(ar.ODD_CLASSES)
    X, plain, names = ar.odd_batch(n, sr, _speech_rows(vb, n, sr, 2 * total))
    assert X.shape[0] == total == 200
    est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    seg = np.arange(total, dtype=np.int64)
    w = oracle.window("hanning", n)
    ordinary = np.array([k == "speech" for k in names])
    rng = np.random.default_rng(77)
    failures = []
    # formants and MFCC do not depend on the pitch setting: the oracle once
    oth = []
    for i in range(total):
        fs, ef, _, _ = oracle.find_formants(X[i], sr, P, est0)
        stable = fs == 0 and ar.formants_stable(oracle, X[i], sr, P, est0, ef, rng)
        ms, em = oracle.mfcc(X[i] * w, 13, 100.0, 8000.0, sr)
        oth.append((fs, ef, stable, ms, em))
    for pitch in ((0.2, 75.0, 600.0), (0.45, 60.0, 2000.0)):
        params = pkg.AnalysisParams.make(sr, pitch=pitch, lpc_order=P, formant_order=P, est_init=est0, mfcc=(13, 100.0, 8000.0))
        rec, st = vb.analyze_frames(X, params, seg_start=seg)
        deferred = vb.last_unsure_count()
        rec_plain, st_plain = vb.analyze_frames(plain, params, seg_start=seg)
        deferred_plain = vb.last_unsure_count()
        c = dict(frames=total, compared=0, ok=0, swap=0, vuv_outside=0, bad=0, status_not_ok=0, formants_compared=0)
        hz = {k: 0 for k in ar.ODD_CLASSES + ["speech"]}
        for i in range(total):
            es, ec, en = oracle.pitch(X[i] * w, sr, pitch[0], pitch[1], pitch[2], cap=2)
            fs, ef, stable, ms, em = oth[i]
            if (st[0, i], st[1, i], st[2, i]) != (es, fs, ms):
                failures.append((pitch, "status", i, names[i], st[:, i].tolist(), (es, fs, ms)))
            if es != 0:
                c["status_not_ok"] += 1
                if not (rec[i, 0] == 0.0 and rec[i, 1] == 0.0):
                    failures.append((pitch, "pair of a frame whose status is not OK", i, names[i], rec[i, 0:2].tolist()))
            else:
                v = ar.classify_top(rec[i, 0:2], ec, en)
                c["compared"] += 1
                c[v] += 1
                if v not in ("ok", "swap"):
                    failures.append((pitch, v, i, names[i], rec[i, 0:2].tolist(), ec.tolist(), en))
            if ms == 0 and np.all(np.isfinite(em)):
                if not np.all(rel_close(rec[i, 10:23], em, 1e-6)):
                    failures.append((pitch, "MFCC", i, names[i], float(np.abs(rec[i, 10:23] - em).max())))
            elif ms == 0 and not np.array_equal(rec[i, 10:23], em, equal_nan=True):          # -inf / NaN coefficients: the same ones
                failures.append((pitch, "MFCC (non-finite)", i, names[i], rec[i, 10:23].tolist(), em.tolist()))
            if fs == 0:
                if not np.all(np.isfinite(rec[i, 2:10])):
                    failures.append((pitch, "formants not finite", i, names[i]))
                if stable:
                    c["formants_compared"] += 1
                    hz[names[i]] += 1
                    if not np.all(np.abs(rec[i, 2:10:2] - ef[:, 0]) <= 1e-4 * np.abs(ef[:, 0]) + 1e-9):
                        failures.append((pitch, "formant Hz", i, names[i], rec[i, 2:10:2].tolist(), ef[:, 0].tolist()))
        if c["swap"] > 1:
            failures.append((pitch, "more than one tie swap", c["swap"]))
        # noise, DC + noise, square + noise and the ordinary frames are well conditioned (the oracle alone decides that): all compared
        for k, want in [(k, 6) for k in ar.WELL_CONDITIONED] + [("speech", 98)]:
            if hz[k] != want:
                failures.append((pitch, "formants of a well-conditioned class not compared", k, hz[k]))
        # the impulses really went through the fallback inside the fused call, and only the degenerate frames did
        if n <= 4096 and not deferred > 0:
            failures.append((pitch, "no frame was deferred"))
        for i in np.flatnonzero(np.array([k == "impulses" for k in names])):
            if not (np.all(np.isfinite(rec[i, 23:36])) and st[2, i] == 0 and np.all(rel_close(rec[i, 10:23], oth[i][4], 1e-6))):
                failures.append((pitch, "record of a deferred frame incomplete", int(i)))
        # the ordinary frames never notice their neighbours
        if not (_same_bits(rec[ordinary], rec_plain[ordinary]) and np.array_equal(st[:, ordinary], st_plain[:, ordinary])):
            rows = np.flatnonzero(ordinary)[np.any(rec[ordinary].view(np.int64) != rec_plain[ordinary].view(np.int64), axis=1)]
            failures.append((pitch, "ordinary rows changed with their neighbours", rows[:8].tolist()))
        c.update(frame_len=n, setting="%g/%g/%g" % pitch, deferred=int(deferred), deferred_without_the_degenerate_frames=int(deferred_plain),
                 formant_hz_compared_by_class=hz)
        REPORT["degenerate"].append(c)
        print(n, pitch, c)
    assert not failures, failures[:6]


def _to_pcm(frames):
    """Each frame quantised to 16 bits the way a WAV writer would (round to nearest, peak 0.9); silence stays silence."""
    peak = np.max(np.abs(frames), axis=1, keepdims=True)
    return np.clip(np.rint(frames / np.where(peak > 0, peak, 1.0) * 0.9 * 32767.0), -32768, 32767).astype(np.int16)


def test_degenerate_frames_as_16_bit_pcm(vb, pkg):
    """The generators that survive quantisation, among ordinary frames, through the native PCM kernel (1,200 samples): bit for bit the
    records of widening first, at both settings."""
    n, sr = 1200, 48000.0
    total = 98 + 6 * len(ar.PCM_CLASSES)
    X, _, names = ar.odd_batch(n, sr, _speech_rows(vb, n, sr, 2 * total), classes=list(ar.PCM_CLASSES))
    pcm = _to_pcm(X).reshape(-1)
    est0 = np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])
    seg = np.arange(total, dtype=np.int64)
    wide = vb.pcm16_to_f64(pcm)
    assert np.array_equal(wide.numpy(), pcm.astype(np.float64) / 32767.0)
    for pitch in ((0.2, 75.0, 600.0), (0.45, 60.0, 2000.0)):
        params = pkg.AnalysisParams.make(sr, pitch=pitch, lpc_order=P, formant_order=P, est_init=est0, mfcc=(13, 100.0, 8000.0))
        a, sa = vb.analyze_frames_pcm16(pcm, params, seg_start=seg, frame_len=n, stride=n)
        deferred = vb.last_unsure_count()
        b, sb = vb.analyze_frames(wide, params, seg_start=seg, frame_len=n, stride=n, n_frames=total)
        assert np.array_equal(sa, sb), (pitch, np.flatnonzero(np.any(sa != sb, axis=0))[:8].tolist())
        rows = np.flatnonzero(np.any(a.view(np.int64) != b.view(np.int64), axis=1))
        assert rows.size == 0, (pitch, rows[:8].tolist(), [names[i] for i in rows[:8]])
        assert deferred > 0 and np.any(sa[1] == 1) and np.count_nonzero(a[:, 0]) > 50      # impulses deferred, silence is Err(LPC), voiced frames
        REPORT["pcm16"].append(dict(case="degenerate frames", setting="%g/%g/%g" % pitch, frames=total, deferred=int(deferred)))
    wide.free()


# ---- the PCM form and non-finite parameters -----------------------------------------------------------------------------------

@pytest.mark.parametrize("pitch", [(0.2, 120.0, 200.0), (1.5, 75.0, 600.0), (0.2, 100.0, 20000.0), (0.0, 75.0, 600.0)], ids=lambda p: "%g-%g-%g" % p)
@pytest.mark.parametrize("n,hop", [(1200, 480), (1024, 512)])
def test_analyze_frames_pcm16_is_bit_identical_to_widening_first_at_other_settings(vb, pkg, n, hop, pitch):
    """test_analyze_frames_pcm16_is_bit_identical_to_widening_first (tests/test_gpu_frontend.py) at pitch settings other than the default:
    the native PCM kernel (1200 / 480) and a shape that is widened inside the library."""
    frames = 700
    d = vb.synth_speech((frames - 1) * hop + n, sample_offset=3 * 48000)
    x = d.numpy()
    d.free()
    pcm = np.clip(np.rint(x / np.max(np.abs(x)) * 0.9 * 32767.0), -32768, 32767).astype(np.int16)
    params = pkg.AnalysisParams.make(48000.0, pitch=pitch)
    seg = np.array([0, 250, 251], dtype=np.int64)
    a, sa = vb.analyze_frames_pcm16(pcm, params, seg_start=seg, frame_len=n, stride=hop)
    wide = vb.pcm16_to_f64(pcm)
    b, sb = vb.analyze_frames(wide, params, seg_start=seg, frame_len=n, stride=hop, n_frames=frames)
    wide.free()
    assert a.shape == (frames, 36) and np.array_equal(sa, sb) and not sa.any()
    rows = np.flatnonzero(np.any(a.view(np.int64) != b.view(np.int64), axis=1))
    assert rows.size == 0, (rows[:5].tolist(), a[rows[0]], b[rows[0]])
    voiced = int(np.count_nonzero(a[:, 0]))
    assert (voiced == 0) if pitch[0] > 1.0 else (voiced > 50), voiced
    REPORT["pcm16"].append(dict(case="%d/%d" % (n, hop), setting="%g/%g/%g" % pitch, frames=frames, voiced=voiced))


@pytest.mark.parametrize("n", [1200, 1024])
def test_nonfinite_and_negative_pitch_parameters(vb, pkg, oracle, bank, n):
    """threshold, fmin, fmax = NaN and a negative fmin through the fused call: whatever status and pair the oracle returns (the
    reference's sort panics on a NaN strength, a comparison with a NaN bound is false, a negative fmin filters nothing).  The oracle is
    asked, nothing is hard-coded; every other column and status stays that of the default setting."""
    shape = (n, 480 if n == 1200 else 512, 48000.0)
    it = bank.get(shape)
    nan = float("nan")
    base = vb.analyze_frames(it["d"], bank.params(shape, ar.DEFAULT_PITCH), frame_len=n, stride=it["stride"], n_frames=F)
    failures = []
    for pitch in ((nan, 75.0, 600.0), (0.2, nan, 600.0), (0.2, 75.0, nan), (0.2, -10.0, 600.0), (nan, nan, nan)):
        rec, st = vb.analyze_frames(it["d"], bank.params(shape, pitch), frame_len=n, stride=it["stride"], n_frames=F)
        _, ost, top2, cnt = ar.oracle_records(oracle, it["x"], n, it["stride"], range(F), 48000.0, pitch, 0, 0, None, None, None)
        c, problems = _judge_pitch(rec[:, 0:2], st[0], ost[0], top2, cnt)
        if not (_same_bits(rec[:, 2:], base[0][:, 2:]) and np.array_equal(st[1:], base[1][1:])):
            problems.append("columns other than pitch differ from the default setting's")
        failures += [(pitch, p) for p in problems]
        REPORT["parameters"].append(dict(shape=_key(shape), setting=repr(pitch), **c))
    assert not failures, failures[:6]


# ---- the record ----------------------------------------------------------------------------------------------------------------

def test_zz_analyze_params_report():
    """Runs last in this file: the caps over the whole file, that no case passed by being trivially unvoiced, and the report."""
    sweep = REPORT["sweep"]
    cases = [c for s in sweep.values() for c in s.values()] + REPORT["instances"] + REPORT["degenerate"] + REPORT["parameters"]
    tot = {k: sum(c[k] for c in cases) for k in ("frames", "compared", "swap", "bad", "vuv_outside", "status_not_ok")}
    tot["not_bitwise_vs_pitch_f64"] = sum(c.get("not_bitwise_vs_pitch_f64", 0) for c in cases)
    tot["deferred_in_degenerate_batches"] = sum(c["deferred"] for c in REPORT["degenerate"])
    voiced_shapes = {name: sum(1 for s in sweep.values() if name in s and s[name]["voiced"] > 0) for name in ar.SETTING_NAMES}
    REPORT["total"], REPORT["shapes_with_voiced_top_candidates_per_setting"] = tot, voiced_shapes
    print("\nfused frame loop across pitch parameters:", json.dumps(tot), json.dumps(voiced_shapes))
    out = os.environ.get("VBX_TEST_REPORT_DIR")          # where to keep the report as a file (profiles/analyze_params/report.json is one)
    if out and os.path.isdir(out):
        with open(os.path.join(out, "analyze_params_report.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1)
    assert tot["bad"] == 0 and tot["vuv_outside"] == 0, tot
    assert tot["swap"] <= tot["compared"] // 500, tot                       # 0.2 % of the frames compared (expected: 0)
    assert tot["compared"] + tot["status_not_ok"] == tot["frames"], tot        # no frame left out
    if len(sweep) == len(ar.SHAPES):                                         # (a run of the whole file)
        for name, k in voiced_shapes.items():
            assert (k == 0) if name in ar.NEVER_VOICED else (k >= 10), (name, k)
