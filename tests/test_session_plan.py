"""vbx_session_plan, the host arithmetic of a live session's push, without a GPU: seeded schedules of block sizes -- single samples,
sub-hop sizes, exact hops, 70-hop blocks -- with utterance marks at random points, at shapes with overlap, without, and with gaps
between the frames.  What is held: the pushes' frame ranges tile the Windower's frames in order, the warm-up is min(lo - utt, 64) and
never reaches before the mark, nothing a push reads was dropped by an earlier one, and the carry never outgrows its buffer."""
import numpy as np
import pytest

SHAPES = [(1200, 480), (1024, 512), (512, 512), (400, 1000), (4, 1)]
WARM = 64


def _schedule(rng, stride, pushes):
    """block sizes: single samples, sub-hop sizes, exact hops and 70-hop blocks, in a seeded order"""
    kinds = rng.integers(0, 5, pushes)
    sizes = []
    for k in kinds:
        if k == 0:
            sizes.append(1)
        elif k == 1:
            sizes.append(int(rng.integers(1, max(2, stride))))
        elif k == 2:
            sizes.append(stride)
        elif k == 3:
            sizes.append(int(rng.integers(1, 3 * stride + 1)))
        else:
            sizes.append(70 * stride)
    return sizes


def _windower_frames(total, frame_len, stride):
    """the Windower's frame starts on `total` samples (src/periodic.rs's user loops: a frame per hop while a whole frame is left)"""
    return [s for s in range(0, total - frame_len + 1, stride)] if total >= frame_len else []


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}/{h}" for n, h in SHAPES])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_schedules(pkg, shape, seed):
    N, H = shape
    rng = np.random.default_rng(1000 * seed + N + H)
    sizes = _schedule(rng, H, 400)
    max_block = max(sizes)
    cap_tail = (WARM + 1) * H + N                               # the carry's capacity minus max_block
    consumed, utt, prev_keep, next_lo = 0, 0, 0, 0
    marks = []
    saw = dict(warm64=False, cont=False, noframe=False, mark_mid=False)
    for n_new in sizes:
        if rng.random() < 0.05:                                 # vbx_session_mark_utterance: the next frame delivered starts an utterance
            utt = pkg.frame_count(consumed, N, H)
            marks.append(utt)
        p = pkg.session_plan(consumed, utt, n_new, N, H)
        lo, hi = pkg.frame_count(consumed, N, H), pkg.frame_count(consumed + n_new, N, H)
        assert (p.lo, p.hi) == (lo, hi) and p.lo == next_lo      # the ranges tile the frames in order
        next_lo = p.hi
        if hi > lo:
            assert p.warm == min(lo - utt, WARM) and lo - p.warm >= utt
            assert p.continues_prev == (1 if lo > utt else 0)
            # every sample the analysis reads is at hand: not dropped before, and consumed by the end of this push
            assert p.read_from == (lo - p.warm) * H and p.read_from >= prev_keep
            assert (hi - 1) * H + N <= consumed + n_new
            saw["warm64"] |= p.warm == WARM
            saw["cont"] |= bool(p.continues_prev)
            saw["mark_mid"] |= 0 < p.warm < WARM
        else:
            assert p.warm == 0 and p.continues_prev == 0
            saw["noframe"] = True
        assert p.keep_from == min(consumed + n_new, (hi - min(hi - utt, WARM)) * H)
        assert p.keep_from >= prev_keep                          # monotone
        assert consumed + n_new - p.keep_from <= cap_tail        # what stays fits beside the next block
        assert consumed + n_new - min(p.read_from, p.keep_from) <= cap_tail + max_block      # ... and what the push holds fits the buffer
        prev_keep = p.keep_from
        consumed += n_new
    assert all(saw.values()), saw
    # the frames are the Windower's: frame f starts at f * stride, and with stride > frame_len the gaps' samples belong to no frame
    starts = _windower_frames(consumed, N, H)
    assert next_lo == len(starts) == pkg.frame_count(consumed, N, H)
    assert all(s == f * H for f, s in enumerate(starts))


def test_gaps_are_dropped(pkg):
    """stride > frame_len: a session that stops inside a gap carries nothing, and the next push's analysis starts inside its block"""
    N, H = 400, 1000
    p = pkg.session_plan(0, 0, 700, N, H)                        # frame 0 complete, 300 samples into the gap
    assert (p.lo, p.hi, p.warm) == (0, 1, 0)
    assert p.keep_from == 0                                      # frame 0 is the next push's warm-up
    p = pkg.session_plan(700, 0, 100, N, H)                      # no frame: still in the gap
    assert (p.lo, p.hi) == (1, 1) and p.keep_from == 0
    pkg_plan = pkg.session_plan(800, 1, 100, N, H)               # a mark at frame 1: frame 0 is no longer needed, the gap is dropped
    assert pkg_plan.keep_from == 900 and (pkg_plan.lo, pkg_plan.hi) == (1, 1)
    p = pkg.session_plan(900, 1, 600, N, H)                      # frame 1 = samples [1000, 1400): it starts 100 samples into the block
    assert (p.lo, p.hi, p.warm, p.continues_prev, p.read_from) == (1, 2, 0, 0, 1000)


def test_hand_checked_values(pkg):
    p = pkg.session_plan(0, 0, 1200, 1200, 480)
    assert p.as_dict() == dict(lo=0, hi=1, warm=0, continues_prev=0, read_from=0, keep_from=0)
    p = pkg.session_plan(1200 + 100 * 480, 0, 70 * 480, 1200, 480)
    assert p.as_dict() == dict(lo=101, hi=171, warm=64, continues_prev=1, read_from=37 * 480, keep_from=107 * 480)
    p = pkg.session_plan(1200 + 100 * 480, 95, 480, 1200, 480)   # an utterance that began 6 frames ago
    assert p.as_dict() == dict(lo=101, hi=102, warm=6, continues_prev=1, read_from=95 * 480, keep_from=95 * 480)
    p = pkg.session_plan(5, 0, 7, 1200, 480)                     # no frame yet: everything is kept
    assert p.as_dict() == dict(lo=0, hi=0, warm=0, continues_prev=0, read_from=0, keep_from=0)


def test_bad_arguments(pkg):
    L = pkg.load_library()
    plan = pkg.SessionPlan()
    import ctypes as C
    assert L.vbx_session_plan(0, 0, 1, 0, 1, C.byref(plan)) == -1        # frame_len 0
    assert L.vbx_session_plan(0, 0, 1, 1, 0, C.byref(plan)) == -1        # stride 0
    assert L.vbx_session_plan(0, 0, 1, 1, 1, None) == -1                 # no output
    assert L.vbx_session_plan(0, 1, 1, 4, 1, C.byref(plan)) == -1        # an utterance that starts beyond the frames consumed
    assert L.vbx_session_plan(2 ** 64 - 1, 0, 2, 4, 1, C.byref(plan)) == -1
    with pytest.raises(pkg.VoxBoxError):
        pkg.session_plan(0, 0, 1, 0, 1)
