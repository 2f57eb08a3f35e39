"""vbx_session_channels_plan, the host arithmetic of one push of a multi-channel live session, without a GPU: over a grid of stream
positions, utterance starts, block sizes (none, one sample, below a hop, one hop, many hops), frame shapes, element sizes and channel
counts, the one-channel fields are vbx_session_plan's, every real frame k Q + j (j < m) of the one frame-loop call reads only samples
of plane k that the ingest writes, every plane base is a multiple of 256 bytes, the segment list is [0, Q, 2Q, ...], and nothing the
call reads lies beyond the stated capacity."""
import itertools

import pytest

SHAPES = [(1200, 480), (1024, 512), (512, 512), (400, 1000)]
WARM = 64


def _grid(N, H):
    """(consumed, utt_frame, n_new): positions before the first frame, inside the warm-up's growth and past its saturation; an
    utterance that began at the stream's start, recently, and exactly at the next frame"""
    for consumed in (0, 1, N - 1, N, N + H - 1, N + 3 * H, N + 70 * H + 7, N + 300 * H + H // 2):
        lo = max(0, (consumed - N) // H + 1) if consumed >= N else 0
        for utt in sorted({0, lo // 2, max(lo - 3, 0), lo}):
            for n_new in (0, 1, max(H // 3, 1), H - 1 if H > 1 else 1, H, H + 1, 10 * H, 100 * H + 5):
                yield consumed, utt, n_new


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}/{h}" for n, h in SHAPES])
@pytest.mark.parametrize("elem", [2, 4, 8])
def test_the_plane_layout_holds_every_real_frame(pkg, shape, elem):
    N, H = shape
    seen = dict(noframe=False, warm64=False, gap=False, many=False)
    for (consumed, utt, n_new), K in itertools.product(_grid(N, H), (1, 2, 5, 64)):
        one = pkg.session_plan(consumed, utt, n_new, N, H)
        cp, seg = pkg.session_channels_plan(consumed, utt, n_new, N, H, elem, K)
        assert cp.push.as_dict() == one.as_dict()
        nf = one.hi - one.lo
        end = consumed + n_new
        m, Q = cp.frames, cp.plane_frames
        assert m == (one.warm + nf if nf else 0)
        assert cp.base == (one.read_from if nf else one.keep_from) and cp.base <= end
        assert cp.keep == max(consumed - cp.base, 0) and cp.len == end - cp.base
        # the layout: Q whole hops per plane, every plane base on a 256-byte boundary, the segment list
        assert Q >= 1 and cp.plane_ld == Q * H and cp.len <= cp.plane_ld == cp.capacity
        assert (cp.plane_ld * elem) % 256 == 0
        assert Q < cp.len // H + 1 + 256                          # no more padding than the alignment asks for
        assert list(seg) == [k * Q for k in range(K)]
        assert cp.call_frames == ((K - 1) * Q + m if m else 0)
        if m:
            assert Q >= m
            # frame k Q + j of the call starts at element (k Q + j) H: inside plane k, within what the ingest wrote there
            first, last = 0, (m - 1) * H + N
            assert first >= 0 and last <= cp.len
            # ... and those elements are the stream's samples [base + j H, base + j H + N) of the frames [lo - warm, hi)
            assert cp.base == (one.lo - one.warm) * H and cp.base + last == (one.hi - 1) * H + N <= end
            # the whole call (its widening pass reads every element up to its last frame's end) stays inside the planes
            assert (cp.call_frames - 1) * H + N <= (K - 1) * cp.plane_ld + cp.len <= K * cp.capacity
        seen["noframe"] |= nf == 0 and n_new > 0
        seen["warm64"] |= one.warm == WARM
        seen["gap"] |= cp.keep == 0 and cp.base > consumed
        seen["many"] |= nf >= 100
    assert seen["noframe"] and seen["warm64"] and seen["many"]
    assert seen["gap"] == (H > N)                                 # frames with gaps between them: the block's first samples are dropped


def test_a_plane_never_outgrows_the_carry(pkg):
    """what vbx_session_open_channels sizes the carry by: a plane of a push of at most max_block sample frames holds at most
    (WARM + 1) * stride + frame_len + max_block elements, so its pitch never exceeds the plan of that many new samples"""
    for (N, H), elem, max_block in itertools.product(SHAPES, (2, 8), (1, 480, 48000)):
        cap = (WARM + 1) * H + N + max_block
        q_max = pkg.session_channels_plan(0, 0, cap, N, H, elem, 3)[0].plane_frames
        consumed = utt = 0
        for step in range(300):
            n_new = (1, H, max_block, max(max_block // 3, 1))[step % 4]
            if step % 37 == 36:
                utt = pkg.frame_count(consumed, N, H)
            cp, _ = pkg.session_channels_plan(consumed, utt, n_new, N, H, elem, 3)
            assert cp.len <= cap and cp.plane_frames <= q_max
            consumed += n_new


def test_bad_arguments(pkg):
    import ctypes as C
    L = pkg.load_library()
    plan = pkg.SessionChannelsPlan()
    ok = (0, 0, 480, 1200, 480, 2, 2)
    assert L.vbx_session_channels_plan(*ok, C.byref(plan), None) == 0
    assert L.vbx_session_channels_plan(*ok, None, None) == -1                                 # no output
    for bad in ((0, 0, 480, 0, 480, 2, 2), (0, 0, 480, 1200, 0, 2, 2), (0, 0, 480, 1200, 480, 3, 2), (0, 0, 480, 1200, 480, 2, 0),
                (0, 0, 480, 1200, 480, 2, 65), (0, 1, 480, 1200, 480, 2, 2)):
        assert L.vbx_session_channels_plan(*bad, C.byref(plan), None) == -1, bad
