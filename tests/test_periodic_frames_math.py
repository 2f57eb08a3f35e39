"""tests/periodic_frames.py on the CPU: the tiling gives identical frames at distance K, and the comparer reports each way a batched
loop goes wrong -- rows shifted by one from a given row on, one stale batch, an unwritten row, a damaged tail row -- and accepts the
clean array.  The stand-in "kernel" is a function of the frame's samples alone."""
import os
import sys

import numpy as np
import pytest

import periodic_frames as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synth():
    p = os.path.join(ROOT, "vox_box.rs_amd")
    if p not in sys.path:
        sys.path.insert(0, p)
    import synth
    return synth.synth_speech


@pytest.mark.parametrize("n,hop,K", [(1200, 480, 37), (4096, 128, 211), (4097, 2048, 37), (2205, 882, 37), (100, 7, 211), (64, 64, 37)])
def test_frames_at_distance_K_are_identical(n, hop, K):
    pf.check_period(K, hop, n)
    pattern = _synth()(K * hop, sample_offset=3 * 48000 + 12345)
    F = 3 * K + 11
    x = pf.tiled(pattern, pf.samples_needed(F, hop, n))
    assert x.size == (F - 1) * hop + n
    frames = np.lib.stride_tricks.sliding_window_view(x, n)[::hop]
    assert frames.shape == (F, n)
    assert np.array_equal(frames[K:], frames[:F - K])
    # and no frame is periodic in itself, nor equal to another of the same period
    first = frames[:K]
    assert len({first[f].tobytes() for f in range(K)}) == K
    assert not np.array_equal(first[0][:n // 2], first[0][n - n // 2:])


def test_check_period_refuses_a_composite_K_and_a_short_pattern():
    with pytest.raises(AssertionError):
        pf.check_period(35, 480, 1200)
    with pytest.raises(AssertionError):
        pf.check_period(37, 64, 1200)
    with pytest.raises(AssertionError):
        pf.assert_batch_breaks_period(37 * 100, 37)
    pf.assert_batch_breaks_period(8190, 37)


K, PER, F = 37, 1000, 2 * 1000 + 437


def _clean(dtype, cols):
    """what a correct batched call leaves in canary_rows(dtype, F + K, cols): row f a function of f % K"""
    rng = np.random.default_rng(7)
    out = pf.canary_rows(dtype, F + K, cols)
    dt = np.dtype(dtype)
    shape = (K,) if cols is None else (K, cols)
    if dt.kind == "i":
        first = (rng.permutation(int(np.prod(shape))) - 5).reshape(shape).astype(dt)      # (counts and statuses; no two rows alike)
    elif dt.kind == "c":
        first = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dt)
    else:
        first = rng.standard_normal(shape).astype(dt)
        first.reshape(K, -1)[5, 0] = np.nan               # a NaN the kernel itself wrote compares equal to itself
    out[:F] = first[np.arange(F) % K]
    return out


SHAPES = [(np.float64, 13), (np.float32, 12), (np.int32, None), (np.complex128, 4), (np.float64, None)]


@pytest.mark.parametrize("dtype,cols", SHAPES)
def test_the_clean_array_passes(dtype, cols):
    pf.assert_periodic("clean", "rows", _clean(dtype, cols), F, K, PER)


@pytest.mark.parametrize("dtype,cols", SHAPES)
def test_rows_shifted_by_one_from_a_row_on_are_reported(dtype, cols):
    a = _clean(dtype, cols)
    a[PER + 1:F] = a[PER:F - 1].copy()                    # the second batch wrote through a pointer one row late
    with pytest.raises(AssertionError, match=rf"breaks the period of {K} frames at row {PER + 1} \(batch 1, position 1 in the batch of {PER}\)"):
        pf.assert_periodic("shift", "rows", a, F, K, PER)


@pytest.mark.parametrize("dtype,cols", SHAPES)
def test_one_stale_batch_is_reported(dtype, cols):
    a = _clean(dtype, cols)
    a[PER:2 * PER] = a[:PER].copy()                       # batch 1 holds batch 0's rows (its scratch indexed by f, or never refilled)
    assert PER % K != 0
    with pytest.raises(AssertionError, match=r"breaks the period .* \(batch 1, position \d+ in the batch"):
        pf.assert_periodic("stale", "rows", a, F, K, PER)


@pytest.mark.parametrize("dtype,cols", SHAPES)
def test_an_unwritten_row_is_reported(dtype, cols):
    a = _clean(dtype, cols)
    a[F - 1] = pf.canary_rows(dtype, 1, cols)[0]          # the short last batch stopped one frame early
    with pytest.raises(AssertionError, match=rf"never written at row {F - 1} \(batch 2, position {F - 1 - 2 * PER} "):
        pf.assert_periodic("unwritten", "rows", a, F, K, PER)


@pytest.mark.parametrize("dtype,cols", SHAPES)
def test_a_damaged_tail_row_is_reported(dtype, cols):
    a = _clean(dtype, cols)
    a[F + 2] = a[2]                                       # the last batch's grid rounded up past F
    with pytest.raises(AssertionError, match=rf"written PAST its {F} rows: tail row 2 \(row {F + 2}\)"):
        pf.assert_periodic("tail", "rows", a, F, K, PER)


def test_padding_columns_must_keep_their_canary():
    a = pf.canary_rows(np.float64, F + K, 14)
    a[:F, :13] = _clean(np.float64, 13)[:F]
    pf.assert_periodic("padded", "rows", a, F, K, PER, written_words=13)
    with pytest.raises(AssertionError, match="never written"):
        pf.assert_periodic("padded", "rows", a, F, K, PER)
    a[PER + 3, 13] = 0.0
    with pytest.raises(AssertionError, match=rf"padding of row {PER + 3} \(batch 1, position 3 "):
        pf.assert_periodic("padded", "rows", a, F, K, PER, written_words=13)
