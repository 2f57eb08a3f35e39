"""Period-K frames: what holds EVERY row of a call of hundreds of thousands of frames from one download and one vectorised comparison.

* `tiled(pattern, n_samples)` repeats a pattern of K * hop samples.  Frame f + K of the Windower view at that hop then holds exactly the
  samples of frame f, whatever the frame length, so a kernel that is a function of the frame's samples writes row f + K == row f, bit
  for bit.  K is prime (37 and 211 are the suite's odd sizes) and the pattern is at least three frame lengths long, so no frame is
  periodic in itself.  `check_period` asserts both; the pattern itself is the caller's (a stretch of synth_speech).
* `canary_rows(dtype, F + K, cols)` is an output image of F rows and K extra ones, pre-filled with layout_arena's canaries.
* `assert_periodic(label, name, rows, F, K, per)` asserts rows[f] == rows[f % K] bit for bit for every f < F (NaN-safe, as
  layout_arena.assert_same_bits), that no compared element still holds a canary, and that the rows past F are untouched.  The message
  names the first bad row, its batch (f // per) and its position in the batch (f % per).  A row shifted across a batch seam, a batch
  that read the previous batch's scratch, a batch that was never written, a short last batch that writes past F: each breaks one of
  the three.

The first K rows are the caller's to hold against a reference; this module says nothing about them.

A precondition: the batch size must not be a multiple of K, or a batch's stale scratch would line up with the period.
`assert_batch_breaks_period(per, K)` asserts it; every case calls it with the batch size the library's probe reports."""
import numpy as np

import layout_arena as la


def is_prime(k):
    return k >= 2 and all(k % d for d in range(2, int(k ** 0.5) + 1))


def check_period(K, hop, frame_len):
    assert is_prime(K), f"K = {K} is not prime"
    assert K * hop >= 3 * frame_len, f"the pattern ({K} * {hop} samples) is shorter than three frames of {frame_len}"


def samples_needed(F, hop, frame_len):
    return (F - 1) * hop + frame_len


def tiled(pattern, n_samples):
    """`pattern` repeated to n_samples samples (any dtype)."""
    pattern = np.ascontiguousarray(pattern)
    assert pattern.ndim == 1 and pattern.size >= 1
    reps = -(-int(n_samples) // pattern.size)
    return np.tile(pattern, reps)[:int(n_samples)]


def assert_batch_breaks_period(per, K):
    assert per > 0 and per % K != 0, f"a batch of {per} frames is a multiple of the period {K}: stale scratch would go unnoticed"


def canary_rows(dtype, rows, cols=None):
    """[rows] or [rows, cols] of `dtype`, every element layout_arena's canary of that type."""
    ut, word = la.canary_of(dtype)
    dt = np.dtype(dtype)
    shape = (rows,) if cols is None else (rows, cols)
    n = int(np.prod(shape)) * (2 if dt.kind == "c" else 1)
    return np.full(n, word, dtype=ut).view(dt).reshape(shape)


def _rows2(a):
    """[rows, words per row] unsigned view of an array whose first axis is the frame."""
    a = np.ascontiguousarray(a)
    w = a.view({2: np.uint16, 4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])
    return w.reshape(a.shape[0], -1) if a.shape[0] else w.reshape(0, 0)


def _where(f, per):
    return f"row {f} (batch {f // per}, position {f % per} in the batch of {per})"


def assert_periodic(label, name, rows, F, K, per, written_words=None):
    """`rows`: [F + tail, ...] as downloaded, tail = 0 or more canary rows the call must not have touched.  written_words: the leading
    words (elements; halves of a pair) of a row that the call writes, where its rows end in padding -- which must still hold the canary."""
    assert rows.shape[0] >= F > K, (label, name, rows.shape, F, K)
    w = _rows2(rows)
    _, word = la.canary_of(rows.dtype)
    tail = w[F:]
    if tail.size and np.any(tail != word):
        r = int(np.argwhere(np.any(tail != word, axis=1))[0][0])
        raise AssertionError(f"{label}: output '{name}' was written PAST its {F} rows: tail row {r} (row {F + r}) no longer holds the canary")
    body = w[:F]
    if written_words is not None and written_words < w.shape[1]:
        pad = body[:, written_words:]
        if np.any(pad != word):
            f = int(np.argmax(np.any(pad != word, axis=1)))
            raise AssertionError(f"{label}: output '{name}' was written in the padding of {_where(f, per)}")
        body = body[:, :written_words]
    blank = np.any(body == word, axis=1)
    if blank.any():
        f = int(np.argmax(blank))
        raise AssertionError(f"{label}: output '{name}' was never written at {_where(f, per)}: {int(blank.sum())} rows still hold a canary")
    # rows[f] against rows[f % K], a block of K rows at a time without an index array of F entries
    first = body[:K]
    bad_row = -1
    n_bad = 0
    for f0 in range(K, F, K * 4096):
        blk = body[f0:min(F, f0 + K * 4096)]
        full = (blk.shape[0] // K) * K
        ne = np.zeros(blk.shape[0], dtype=bool)
        if full:
            ne[:full] = np.any(blk[:full].reshape(-1, K, blk.shape[1]) != first[None], axis=2).reshape(-1)
        if blk.shape[0] > full:
            ne[full:] = np.any(blk[full:] != first[:blk.shape[0] - full], axis=1)
        if ne.any():
            n_bad += int(ne.sum())
            if bad_row < 0:
                bad_row = f0 + int(np.argmax(ne))
    if bad_row >= 0:
        col = int(np.argmax(body[bad_row] != first[bad_row % K]))
        raise AssertionError(f"{label}: output '{name}' breaks the period of {K} frames at {_where(bad_row, per)}: it differs from row "
                             f"{bad_row % K} (first at word {col}); {n_bad} rows differ in all")
