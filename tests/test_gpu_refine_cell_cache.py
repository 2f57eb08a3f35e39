"""The wave-wide Brent refinement with its two unit cells' samples held in registers, pinned bit for bit on an input that
walks the top lag through every integer from 80 to 640: sha-256 of vbx_pitch_f64's lists at kmax 1, 2 and 3, of the fused
record at 1200/480 from f64, 16-bit PCM and float32 samples, and of lists and record at 1024/512, 2048/1024 and 4096/2048.

Input (glide_pcm): a tone with weak noise whose PERIOD grows linearly from 80 to 640 samples (600 Hz down to 75 Hz at
48 kHz) over 1,200 frames, followed by 64 frames of noise alone; the longer shapes take the same glide stretched in time
(1,200 frames of their own hop).  A lag of L sums L + 2 sinc terms per side, i.e. (L + 2) / 128 whole blocks of four in
every lane and one more, masked, in the lanes with a term to spare: the glide covers 0 to 4 whole blocks (5 with the masked
one), every boundary of the number of blocks kept in registers from both sides, and lags below 126 whose terms are all in
the tail.  The samples
are quantised to 16 bits before anything is computed from them, so the input does not depend on the last bit of the host's
sine; the noise is an integer hash.

tests/golden/refine_cell_digests.json holds the digests of the build BEFORE the samples moved into registers;
tools/record_refine_cell_digests.py writes it (only ever from a build whose outputs are the accepted ones).

tools/experiments/brent_cells.py replays the Brent runs of this input on the CPU oracle
(profiles/refine_cell_cache/brent_cells.txt): at 1200/480 the top candidate's lag runs from 82 to 597 (a 1200-sample frame
searches lags below 600; the longer shapes go on to 640) with 0, 1, 2, 3 and 4 whole blocks per lane, every run visits exactly
two cells, and NO run of this input visits a third cell or takes an exact-integer early-out: those two paths are not
exercised here, and nothing is asserted on them.

Needs a real MI355X: run with `-m gpu`.
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 48000.0
GLIDE_FRAMES = 1200
NOISE_FRAMES = 64
LAG_FROM, LAG_TO = 80.0, 640.0
SHAPES = [(1200, 480), (1024, 512), (2048, 1024), (4096, 2048)]      # frame_len, hop; the first also as PCM16 and float32
KMAX = (1, 2, 3)
GOLDEN = "refine_cell_digests.json"


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hash_noise(count, seed):
    """uniform in [-1, 1), a pure integer hash of the sample index (splitmix64): the same on every host"""
    with np.errstate(over="ignore"):
        z = np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


def glide_pcm(n, hop):
    """int16 samples of GLIDE_FRAMES + NOISE_FRAMES frames of n samples, hop apart"""
    frames = GLIDE_FRAMES + NOISE_FRAMES
    total = (frames - 1) * hop + n
    glide = (GLIDE_FRAMES - 1) * hop + n
    s = np.arange(total, dtype=np.float64)
    lag = LAG_FROM + (LAG_TO - LAG_FROM) * np.minimum(s / float(glide), 1.0)      # the period, in samples
    phase = 2.0 * np.pi * np.cumsum(1.0 / lag)
    tone = 0.5 * np.sin(phase) + 0.2 * np.sin(2.0 * phase + 0.7)
    noise = _hash_noise(total, 0x5EED + n)
    x = np.where(s < glide, tone + 0.01 * noise, 0.3 * noise)
    return np.round(x * 32767.0 * 0.9).astype(np.int16), frames


def _params(pkg):
    return pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=0, mfcc=(13, 100.0, 8000.0))


def _record(rec, st3, params, tag):
    d = {"%s_%s" % (tag, name): _sha(rec[:, c0:c0 + w]) for name, (c0, w) in params.columns().items()}
    d[tag + "_status"] = _sha(st3)
    return d


def compute_digests(vb, pkg):
    out = {}
    for n, hop in SHAPES:
        pcm, frames = glide_pcm(n, hop)
        x = pcm.astype(np.float64) / 32767.0
        d = {"frames": int(frames)}
        audio = vb.to_device(x)
        han = vb.window(pkg.WINDOW_HANNING, n)
        for k in KMAX:
            cand, cnt, st = vb.pitch(audio, SR, 0.2, 75.0, 600.0, kmax=k, frame_len=n, stride=hop, n_frames=frames, window=han)
            assert cand.shape == (frames, k, 2)
            d["pitch_k%d" % k] = _sha(cand)
            d["count_k%d" % k] = _sha(cnt)
            d["status_k%d" % k] = _sha(st)
        params = _params(pkg)
        rec, st3 = vb.analyze_frames(audio, params, frame_len=n, stride=hop, n_frames=frames)
        d.update(_record(rec, st3, params, "record"))
        audio.free()
        if (n, hop) == SHAPES[0]:
            rec, st3 = vb.analyze_frames_pcm16(pcm, params, frame_len=n, stride=hop, n_frames=frames)
            d.update(_record(rec, st3, params, "pcm16"))
            rec, st3 = vb.analyze_frames_ex_f32in(x.astype(np.float32), params, frame_len=n, stride=hop, n_frames=frames)
            d.update(_record(rec, st3, params, "f32in"))
        out["glide %d/%d" % (n, hop)] = d
    return out


def test_cell_cache_outputs_keep_the_parent_builds_digests(vb, pkg, golden_dir):
    with open(os.path.join(golden_dir, GOLDEN)) as f:
        want = json.load(f)["digests"]
    got = compute_digests(vb, pkg)
    assert sorted(got) == sorted(want)
    differ = ["%s: %s" % (shape, k) for shape in want for k in want[shape] if got[shape].get(k) != want[shape][k]]
    for shape in want:
        print(shape, want[shape]["frames"], "frames:", "identical" if not any(s.startswith(shape + ":") for s in differ) else "DIFFER")
    assert not differ, differ
    assert all(sorted(got[s]) == sorted(want[s]) for s in want)
