"""The fenced arena of the layout tests (tests/layout_arena.py) must bite: numpy stand-ins for a kernel that behaves, one
that writes one element past its output, one that writes one element before it, one that writes into a padding column and
one whose result uses the sample just past the frame.  The helper passes the first and flags each of the others, naming
the buffer and the offset.  No GPU: the arena's host backend has the device backend's layout logic."""
import numpy as np
import pytest

import layout_arena as la

F, N, LAGS, LD = 5, 24, 3, 6


def _frames():
    rng = np.random.default_rng(7)
    return rng.uniform(-1.0, 1.0, (F, N))


def _arena(x_res=0, out_res=0, ld=LD, stride=N):
    be = la.HostBackend()
    a = la.Arena(be, label=f"x%16={x_res} out%16={out_res} ld={ld} stride={stride}")
    fr = _frames()
    a.input("x", la.gapped_view(fr, stride), residue=x_res)
    a.output("r", np.float64, F, LAGS, ld=ld, residue=out_res)
    a.output("count", np.int32, F, 1, residue=4 if out_res else 0)
    return a.place(), be, fr


def _lag_sums(be, x_addr, out_addr, count_addr, stride, ld, reach=N, first_row=0, extra_col=None):
    """Stand-in kernel: r[f, k] = sum_i x[i] x[i + k] over one frame (i + k < reach), count[f] = k written."""
    for f in range(F):
        x = be.view(x_addr + f * stride * 8, np.float64, reach + 1)[:reach]
        row = be.view(out_addr + (first_row + f) * ld * 8, np.float64, LAGS)
        for k in range(LAGS):
            row[k] = np.sum(x[:reach - k] * x[k:reach])
        be.view(count_addr + f * 4, np.int32, 1)[0] = LAGS
    if extra_col is not None:
        be.view(out_addr + (2 * ld + extra_col) * 8, np.float64, 1)[0] = 1.0


def _reference(fr):
    return np.array([[np.sum(fr[f, :N - k] * fr[f, k:]) for k in range(LAGS)] for f in range(F)])


@pytest.mark.parametrize("x_res,out_res,ld,stride", [(0, 0, LAGS, N), (8, 8, LD, N), (8, 0, LD, N + 5), (0, 8, LAGS + 1, N + 1)])
def test_a_kernel_that_behaves_passes(x_res, out_res, ld, stride):
    a, be, fr = _arena(x_res, out_res, ld, stride)
    assert a["x"] % 16 == x_res and a["r"] % 16 == out_res and a["count"] % 16 == (4 if out_res else 0)
    _lag_sums(be, a["x"], a["r"], a["count"], stride, ld)
    out = a.finish()
    want = _reference(fr)
    la.assert_same_bits(a.label, "r", out["r"], want)
    la.assert_no_new_nan(a.label, "r", out["r"], want)
    la.assert_written(a.label, "r", out["r"])
    assert np.all(out["count"] == LAGS)


def test_one_element_past_the_output_is_flagged():
    a, be, _ = _arena(8, 8)
    _lag_sums(be, a["x"], a["r"], a["count"], N, LD)
    be.view(a["r"] + ((F - 1) * LD + LAGS) * 8, np.float64, 1)[0] = 0.0          # a zero-fill loop that runs one entry too far
    with pytest.raises(la.ArenaViolation) as e:
        a.finish()
    assert "'r'" in str(e.value) and "PAST its end" in str(e.value) and "(element 0)" in str(e.value), str(e.value)


def test_one_element_before_the_output_is_flagged():
    a, be, _ = _arena(0, 8)
    _lag_sums(be, a["x"], a["r"], a["count"], N, LD)
    be.view(a["r"] - 8, np.float64, 1)[0] = 0.0
    with pytest.raises(la.ArenaViolation) as e:
        a.finish()
    assert "'r'" in str(e.value) and "(1 elements) BEFORE its start" in str(e.value), str(e.value)


def test_a_write_into_a_padding_column_is_flagged():
    a, be, _ = _arena(0, 0)
    _lag_sums(be, a["x"], a["r"], a["count"], N, LD, extra_col=LAGS + 1)
    with pytest.raises(la.ArenaViolation) as e:
        a.finish()
    assert "'r'" in str(e.value) and f"padding column {LAGS + 1} of row 2" in str(e.value), str(e.value)


def test_a_wrong_leading_dimension_is_flagged():
    """Rows written with ld = LAGS into a buffer whose ld is LD land in the padding of the first rows."""
    a, be, _ = _arena(0, 0)
    _lag_sums(be, a["x"], a["r"], a["count"], N, LAGS)
    with pytest.raises(la.ArenaViolation) as e:
        a.finish()
    assert "padding column" in str(e.value)


@pytest.mark.parametrize("stride", [N, N + 3])
def test_a_result_that_uses_the_sample_past_the_frame_is_flagged(stride):
    """Dense batch: only the LAST frame's neighbour is a fence (the others read the next frame: the value changes, no NaN);
    gapped view: every frame's is.  Both are caught: bits differ from the canonical result, and the NaN names the cause."""
    a, be, fr = _arena(8, 0, LD, stride)
    _lag_sums(be, a["x"], a["r"], a["count"], stride, LD, reach=N + 1)
    out = a.finish()                                             # no fence was WRITTEN: the arena itself is intact
    want = _reference(fr)
    with pytest.raises(AssertionError) as e:
        la.assert_no_new_nan(a.label, "r", out["r"], want)
    assert "'r'" in str(e.value) and "input fence" in str(e.value), str(e.value)
    with pytest.raises(AssertionError):
        la.assert_same_bits(a.label, "r", out["r"], want)
    d = la.new_nans(out["r"], want)
    assert d[0][0] == (0 if stride > N else F - 1), d              # the first frame whose neighbour is a fence


def test_an_input_that_is_overwritten_is_flagged():
    a, be, _ = _arena()
    be.view(a["x"] + 16, np.float64, 1)[0] = 3.0
    with pytest.raises(la.ArenaViolation) as e:
        a.finish()
    assert "input 'x': element 2" in str(e.value)


def test_an_output_that_was_never_written_is_flagged():
    a, be, _ = _arena()
    out = a.finish()
    with pytest.raises(AssertionError) as e:
        la.assert_written(a.label, "r", out["r"])
    assert "never written" in str(e.value)
    assert la.unwritten(out["count"]).shape[0] == F


@pytest.mark.parametrize("dtype,residues", [(np.float64, (0, 8)), (np.float32, (0, 4, 8, 12)), (np.int32, (0, 4, 8, 12)),
                                            (np.int16, (0, 2)), (np.complex128, (0, 8)), (np.complex64, (0, 4, 8, 12))])
def test_residues_fences_and_canaries(dtype, residues):
    for res in residues:
        be = la.HostBackend()
        a = la.Arena(be, "residues")
        a.input("in", np.arange(10).astype(dtype), residue=res)
        a.output("out", dtype, 3, 5, ld=7, residue=res)
        a.place()
        assert a["in"] % 16 == res and a["out"] % 16 == res
        b_in, b_out = a.bufs["in"], a.bufs["out"]
        assert b_in.fence_lo >= la.FENCE_MIN and b_out.fence_lo >= la.FENCE_MIN
        assert b_out.off - b_in.off - b_in.nbytes >= 2 * la.FENCE_MIN
        es = np.dtype(dtype).itemsize
        before = be.view(a["in"] - es, dtype, 1)[0]
        after = be.view(a["in"] + 10 * es, dtype, 1)[0]
        if np.dtype(dtype).kind in "fc":
            assert np.isnan(before) and np.isnan(after)
        elif dtype == np.int16:
            assert before == la.PCM_FENCE and after == la.PCM_FENCE
        out = a.finish()["out"]
        assert la.unwritten(out).shape[0] == out.size * (2 if np.dtype(dtype).kind == "c" else 1)
        if np.dtype(dtype).kind in "fc":
            assert np.all(np.isnan(out))


def test_inout_buffers_come_back():
    be = la.HostBackend()
    a = la.Arena(be, "inout")
    data = np.arange(12, dtype=np.float64).reshape(3, 4)
    a.input("rows", data, residue=8, inout=True)
    a.place()
    be.view(a["rows"], np.float64, 12)[:] *= 2.0
    out = a.finish()
    assert np.array_equal(out["rows"], 2.0 * data)
