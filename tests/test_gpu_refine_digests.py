"""The pitch refinement's outputs pinned bit for bit: sha-256 of the candidate lists (kmax 1, 3 and 8), counts and statuses
of vbx_pitch_f64, and of the fused call's record, on a fixed seeded stretch of the synthetic recording at 1200/480, 1024/512
and 4096/2048 and on sample-two_vowels.wav at 1103/441.

The refinement (vbx_pitch_refine.hpp) is reworked for speed under the rule that every output keeps every bit; between two
builds that property was only checked by tools/experiments/bitcompare_libs.py, which needs both libraries side by side.
tests/golden/refine_digests.json holds the digests of the build BEFORE the per-evaluation rework of the wave-wide Brent
iteration; tools/record_refine_digests.py writes it (only ever from a build whose outputs are the accepted ones).

kmax 1 and 3 take the one-candidate-per-wavefront refinement, kmax 8 the grouped one (four or eight candidates side by
side); the fused record takes the first inside analyze_kernel.

Needs a real MI355X: run with `-m gpu`.
"""
import hashlib
import json
import os
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 48000.0
SEED_OFFSET = 7 * 48000 + 4321            # where the stretch starts in the synthetic recording (default seed)
SYNTH_SHAPES = [(1200, 480, 6000), (1024, 512, 6000), (4096, 2048, 1500)]     # frame_len, hop, frames
WAV_SHAPE = (1103, 441)
KMAX = (1, 3, 8)
GOLDEN = "refine_digests.json"


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _pitch_digests(vb, pkg, audio, sr, n, hop, frames):
    han = vb.window(pkg.WINDOW_HANNING, n)
    d = {"frames": int(frames)}
    for k in KMAX:
        cand, cnt, st = vb.pitch(audio, sr, 0.2, 75.0, 600.0, kmax=k, frame_len=n, stride=hop, n_frames=frames, window=han)
        assert cand.shape == (frames, k, 2)
        d["pitch_k%d" % k] = _sha(cand)
        d["count_k%d" % k] = _sha(cnt)
        d["status_k%d" % k] = _sha(st)
    return d


def _record_digest(vb, pkg, audio, sr, n, hop, frames):
    params = pkg.AnalysisParams.make(sr, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=0, mfcc=(13, 100.0, 8000.0))
    rec, st3 = vb.analyze_frames(audio, params, frame_len=n, stride=hop, n_frames=frames)
    d = {"record_" + name: _sha(rec[:, c0:c0 + w]) for name, (c0, w) in params.columns().items()}
    d["record_status"] = _sha(st3)
    return d


def compute_digests(vb, pkg, golden_dir):
    out = {}
    for n, hop, frames in SYNTH_SHAPES:
        audio = vb.synth_speech((frames - 1) * hop + n, sample_offset=SEED_OFFSET)
        d = _pitch_digests(vb, pkg, audio, SR, n, hop, frames)
        d.update(_record_digest(vb, pkg, audio, SR, n, hop, frames))
        audio.free()
        out["synth %d/%d" % (n, hop)] = d
    with wave.open(os.path.join(golden_dir, "sample-two_vowels.wav"), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        sr = float(w.getframerate())
    samples = pcm.astype(np.float64) / 32767.0
    n, hop = WAV_SHAPE
    frames = (samples.size - n) // hop + 1
    d = _pitch_digests(vb, pkg, samples, sr, n, hop, frames)
    d.update(_record_digest(vb, pkg, samples, sr, n, hop, frames))
    out["two_vowels %d/%d" % (n, hop)] = d
    return out


def test_refinement_outputs_keep_their_recorded_digests(vb, pkg, golden_dir):
    with open(os.path.join(golden_dir, GOLDEN)) as f:
        want = json.load(f)["digests"]
    got = compute_digests(vb, pkg, golden_dir)
    assert sorted(got) == sorted(want)
    differ = ["%s: %s" % (shape, k) for shape in want for k in want[shape] if got[shape].get(k) != want[shape][k]]
    for shape in want:
        print(shape, want[shape]["frames"], "frames:", "identical" if not any(s.startswith(shape + ":") for s in differ) else "DIFFER")
    assert not differ, differ
    assert all(sorted(got[s]) == sorted(want[s]) for s in want)
