"""The reference for one record of the fused frame loop (vbx_analyze_frames_f64 / _pcm16): the per-frame loop a user of the
crate writes (include/voxbox_hip.h, "the user's frame loop"), run on the CPU oracle for ARBITRARY parameters, and the rule by
which a record's pitch pair is judged against the oracle's candidate list -- the rule of tests/test_gpu_parity.py::_check_pitch,
so the fused record's pitch column and the stand-alone vbx_pitch_f64 are held to the same thing.

A plain module that tests import (no fixtures, nothing collected).  It needs numpy and the oracle module only, so the CPU tests
of tests/test_analyze_reference.py exercise it without a GPU."""
import numpy as np

# the sweep of tests/test_gpu_analyze_params.py: one (frame_len, hop, sample_rate) per form the fused call can take
SHAPES = [(1200, 480, 48000.0),                                  # the native 1200-point plan
          (800, 320, 48000.0),                                   # padded into it (2400 = 3 * 800)
          (1103, 441, 44100.0), (1600, 640, 22050.0),            # MFCC bins interpolated from the transform's
          (1024, 512, 48000.0), (512, 256, 16000.0),             # the power-of-two 1024 plan, and a frame padded into it
          (2048, 1024, 48000.0),
          (4096, 2048, 96000.0), (3000, 1200, 48000.0), (2205, 882, 44100.0),     # the 4096 plan as two kernels, even and odd
          (256, 128, 8000.0), (400, 160, 16000.0),               # no fused kernel
          (5000, 2000, 48000.0)]                                 # longer than every transform
DEFAULT_PITCH = (0.2, 75.0, 600.0)
SWEEP_FRAMES = 48


def pitch_edge(frame_len, sample_rate):
    """The fmin whose reach 2 ceil(sr / fmin) + 16 lies just below the frame (test_pitch_cut_lag_curve_changes_nothing)."""
    return 2.0 * sample_rate / (frame_len - 40)


def settings(frame_len, sample_rate):
    """(threshold, fmin, fmax) of the sweep.  What each one steers is said in tests/test_gpu_analyze_params.py."""
    return [(0.45, 60.0, 400.0), (0.0, 75.0, 600.0), (0.2, 120.0, 200.0), (0.2, 50.0, 1000.0), (0.2, 100.0, 20000.0),
            (0.9, 75.0, 600.0), (1.5, 75.0, 600.0), (0.2, 300.0, 200.0), (0.2, 0.0, 600.0),
            (0.2, pitch_edge(frame_len, sample_rate), 600.0), (0.2, 400.0, sample_rate)]


SETTING_NAMES = ["0.45/60/400", "0.0/75/600", "0.2/120/200", "0.2/50/1000", "0.2/100/20000", "0.9/75/600", "1.5/75/600",
                 "0.2/300/200", "0.2/0/600", "0.2/edge/600", "0.2/400/sr"]
NEVER_VOICED = ("1.5/75/600", "0.2/300/200")      # a threshold above every strength; an empty band


def sweep_stride(frame_len, sample_rate, frames=SWEEP_FRAMES):
    """The sweep's 48 frames span five seconds of the synthetic recording: the 90-250 Hz glide and the noise-only second."""
    return (int(5 * sample_rate) - frame_len) // (frames - 1)


def sweep_samples(frame_len, sample_rate):
    """(n_samples, sample_offset) of the sweep's signal, for synth_speech on the device or on the host."""
    return int(5 * sample_rate) + frame_len, int(2 * sample_rate)


def mfcc_band(sample_rate):
    return (13, 100.0, min(8000.0, 0.45 * sample_rate))


def record_columns(n_est, lpc_order, formant_order, mfcc):
    """name -> (first column, width), as AnalysisParams.columns() lays the record out."""
    cols, c = {"pitch": (0, 2)}, 2
    if formant_order:
        cols["formants"] = (c, 2 * n_est); c += 2 * n_est
    if mfcc:
        cols["mfcc"] = (c, int(mfcc[0])); c += int(mfcc[0])
    if lpc_order:
        cols["lpc"] = (c, lpc_order + 1); c += lpc_order + 1
    cols["_width"] = (c, 0)
    return cols


def oracle_records(oracle, samples, frame_len, hop, frames, sample_rate, pitch, lpc_order, formant_order, est_init, mfcc, seg):
    """The user's frame loop on the CPU oracle.  `frames`: the frame indices to compute, in the order given (frame t is
    samples[t * hop : t * hop + frame_len]); `seg`: the frame indices at which a segment starts (the tracker's estimates are
    reset to est_init there).  The formant estimates are carried from one listed frame to the next, so for the formant columns
    a caller lists every frame of a segment from its start up to the last one it wants; pitch, MFCC and LPC need no order.
    pitch = (threshold, fmin, fmax) or None; lpc_order / formant_order 0 and mfcc None skip that part (its status stays 0).

    Returns (records [len(frames), width], status [3, len(frames)] = pitch / formant / mfcc, top2 [len(frames), 2, 2] = the
    oracle's two best pitch candidates (frequency, strength; zeros beyond the count), counts [len(frames)])."""
    frames = [int(t) for t in frames]
    seg = set(int(s) for s in (seg if seg is not None else ()))
    est0 = np.asarray(est_init, dtype=np.float64).reshape(-1, 2) if formant_order else np.zeros((0, 2))
    cols = record_columns(est0.shape[0], lpc_order, formant_order, mfcc)
    F = len(frames)
    rec = np.zeros((F, cols["_width"][0]))
    st = np.zeros((3, F), dtype=np.int32)
    top2 = np.zeros((F, 2, 2))
    counts = np.zeros(F, dtype=np.int64)
    w = oracle.window("hanning", frame_len)
    est = est0.copy()
    for i, t in enumerate(frames):
        fr = np.asarray(samples[t * hop:t * hop + frame_len], dtype=np.float64)
        assert fr.size == frame_len, (t, fr.size)
        xw = fr * w
        if pitch is not None:
            s, c, n = oracle.pitch(xw, sample_rate, pitch[0], pitch[1], pitch[2], cap=2)
            st[0, i], counts[i] = s, n
            top2[i, :c.shape[0]] = c
            if c.shape[0]:
                rec[i, 0:2] = c[0]
        if formant_order:
            if t in seg or i == 0:
                est = est0.copy()
            s, est, _, _ = oracle.find_formants(fr, sample_rate, formant_order, est)
            st[1, i] = s
            c0, cw = cols["formants"]
            rec[i, c0:c0 + cw] = est.reshape(-1)
        if mfcc:
            s, m = oracle.mfcc(xw, int(mfcc[0]), mfcc[1], mfcc[2], sample_rate)
            st[2, i] = s
            c0, cw = cols["mfcc"]
            rec[i, c0:c0 + cw] = m
        if lpc_order:
            c0, cw = cols["lpc"]
            rec[i, c0:c0 + cw] = oracle.lpc(oracle.autocorrelate(xw, lpc_order + 1), lpc_order)
    return rec, st, top2, counts


def classify_top(got_pair, ec, en):
    """The top-candidate rule of _check_pitch.  got_pair: (frequency, strength) under test; ec: the oracle's candidates, best
    first (at least its two best where it has two); en: the oracle's candidate count.
      "ok"           frequency within 1e-4 relative and strength within 1e-4 of the oracle's best;
      "swap"         otherwise, the oracle's two best strengths are closer than 1e-3 AND got_pair is the oracle's runner-up
                     (frequency within 1e-4 relative, strength within 1e-3) -- a tie decided the other way; a swap between a
                     voiced candidate and the unvoiced one is one only inside a 1e-4 tie,
      "vuv_outside"  and this otherwise: a voiced / unvoiced decision changed outside the tolerance;
      "bad"          any other disagreement."""
    ec = np.asarray(ec, dtype=np.float64)
    top_ok = abs(got_pair[0] - ec[0, 0]) <= 1e-4 * abs(ec[0, 0]) and abs(got_pair[1] - ec[0, 1]) <= 1e-4
    if top_ok:
        return "ok"
    gap = abs(ec[0, 1] - ec[1, 1]) if en > 1 else np.inf
    is_runner_up = en > 1 and abs(got_pair[0] - ec[1, 0]) <= 1e-4 * abs(ec[1, 0]) and abs(got_pair[1] - ec[1, 1]) <= 1e-3
    if gap < 1e-3 and is_runner_up:
        if (got_pair[0] == 0.0) != (ec[0, 0] == 0.0) and gap > 1e-4:
            return "vuv_outside"
        return "swap"
    return "bad"


def tie_gap(ec, en):
    """The distance between the oracle's two best strengths (inf where it has fewer than two)."""
    return abs(ec[0][1] - ec[1][1]) if en > 1 else np.inf


# ---- degenerate frames (tests/test_gpu_analyze_params.py, section "degenerate frames through the fused call") ------------------

# the generators of test_pitch_odd_signals and test_mfcc_and_formants_odd_signals (tests/test_gpu_parity.py), by name, plus one
# frame with a NaN and one with an Inf sample; PCM_CLASSES are the ones that survive a 16-bit quantisation
ODD_CLASSES = ["noise", "tone", "tone_wide", "square", "chirp", "impulses", "dc_noise", "tiny_tone", "huge_tone", "am_tone_noise",
               "clipped_tone", "silence", "tiny_noise", "huge_tone_440", "square_noise", "nan_sample", "inf_sample"]
PCM_CLASSES = ("noise", "tone", "tone_wide", "square", "chirp", "impulses", "dc_noise", "am_tone_noise", "clipped_tone", "silence",
               "square_noise")
WELL_CONDITIONED = ("noise", "dc_noise", "square_noise")      # test_mfcc_and_formants_odd_signals: every such frame's formants are compared


def odd_frame(name, n, sample_rate, rng, speech_frame):
    """One frame of class `name`; speech_frame: an ordinary frame for the classes that spoil one sample of it."""
    t = np.arange(n) / sample_rate
    if name == "noise":
        return rng.standard_normal(n)
    if name == "tone":
        return np.sin(2 * np.pi * rng.uniform(60, 700) * t + rng.uniform(0, 6))
    if name == "tone_wide":
        return np.sin(2 * np.pi * rng.uniform(60, 7000) * t)
    if name == "square":
        return np.sign(np.sin(2 * np.pi * rng.uniform(80, 400) * t))
    if name == "chirp":
        return np.sin(2 * np.pi * (100 + 3000 * t) * t)
    if name == "impulses":
        return np.bincount(rng.integers(0, n, 5), minlength=n).astype(np.float64)
    if name == "dc_noise":
        return 0.5 + 0.01 * rng.standard_normal(n)
    if name == "tiny_tone":
        return 1e-150 * np.sin(2 * np.pi * 200 * t)
    if name == "huge_tone":
        return 1e120 * np.sin(2 * np.pi * 150 * t)
    if name == "am_tone_noise":
        return np.sin(2 * np.pi * 120 * t) * (1 + 0.5 * np.sin(2 * np.pi * 7 * t)) + 0.2 * rng.standard_normal(n)
    if name == "clipped_tone":
        return np.clip(3 * np.sin(2 * np.pi * rng.uniform(75, 600) * t), -1, 1)
    if name == "silence":
        return np.zeros(n)
    if name == "tiny_noise":
        return 1e-120 * rng.standard_normal(n)
    if name == "huge_tone_440":
        return 1e100 * np.sin(2 * np.pi * 440 * t)
    if name == "square_noise":
        return np.sign(np.sin(2 * np.pi * 150 * t)) + 0.1 * rng.standard_normal(n)
    x = np.array(speech_frame, dtype=np.float64)
    if name == "nan_sample":
        x[100] = np.nan
    elif name == "inf_sample":
        x[7] = np.inf
    else:
        raise ValueError(name)
    return x


def odd_batch(n, sample_rate, speech, classes=ODD_CLASSES, per_class=6, ordinary=98, seed=20251016):
    """A shuffled batch of ordinary frames (rows of `speech`, [at least twice the batch's frames, n]) and degenerate ones, and the same
    batch with every degenerate frame replaced by an ordinary one.  Returns (X, X_plain, names): names[i] is the class of X[i], or
    "speech"."""
    rng = np.random.default_rng(seed + n)
    names = ["speech"] * ordinary + [c for c in classes for _ in range(per_class)]
    order = rng.permutation(len(names))
    names = [names[i] for i in order]
    assert speech.shape[0] >= 2 * len(names) and speech.shape[1] == n
    X = np.zeros((len(names), n))
    plain = np.zeros_like(X)
    for i, name in enumerate(names):
        plain[i] = speech[i]
        X[i] = speech[i] if name == "speech" else odd_frame(name, n, sample_rate, rng, speech[len(names) + i])
    return X, plain, names


def formants_stable(oracle, frame, sample_rate, order, est0, ef, rng):
    """The stability probe of test_mfcc_and_formants_odd_signals: the oracle's own formant Hz survive a 1e-13 perturbation of the
    frame to 1e-7 (pure tones, impulses and 1e100 tones give a Burg polynomial with clustered roots that move by percents: for
    those frames no implementation, the reference included, has digits to compare)."""
    probe = frame * (1.0 + 1e-13 * rng.standard_normal(frame.size))
    ps, pf, _, _ = oracle.find_formants(probe, sample_rate, order, est0)
    return ps == 0 and bool(np.all(np.abs(pf[:, 0] - ef[:, 0]) <= 1e-7 * np.abs(ef[:, 0]) + 1e-12))
