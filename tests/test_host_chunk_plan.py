"""vbx_host_chunk_plan: the chunks vbx_analyze_host cuts a host-resident recording into -- pure host arithmetic, checked here
against the definitions: the chunks tile the frames in order, a warm-up never reaches before the cut utterance's start, the
continues flags name exactly the cuts that lie inside an utterance, and the uploaded samples are those of frames [lo - warm, hi)."""
import numpy as np
import pytest

WARM = 64                                   # VBX_SHARD_WARM_FRAMES
N, H = 1200, 480
SEGS = {"none": None, "five": [0, 150, 200, 390, 600], "every frame": "all"}


def _seg(kind, F):
    s = SEGS[kind]
    if s is None:
        return None
    if isinstance(s, str):
        return np.arange(F, dtype=np.int64)
    return np.array([v for v in s if v <= F], dtype=np.int64)     # (a start beyond the recording is a bad list)


def _chunks(pkg, F, cf, seg):
    nc = -(-F // cf)
    return [pkg.host_chunk_plan(F, cf, c, N, H, seg) for c in range(nc)]


@pytest.mark.parametrize("kind", list(SEGS))
@pytest.mark.parametrize("F", [1, 63, 64, 65, 650, 12_000])
def test_chunks_tile_the_recording(pkg, F, kind):
    seg = _seg(kind, F)
    starts = {0} if seg is None else set(int(v) for v in seg)
    n_samples = (F - 1) * H + N
    for cf in sorted({64, 200, F, F + 1}):
        plans = _chunks(pkg, F, cf, seg)
        assert len(plans) == -(-F // cf)
        at = 0
        for c, (pl, s0, s1) in enumerate(plans):
            label = (F, cf, kind, c)
            # the own ranges tile [0, F) in order
            assert pl.lo == at == c * cf and pl.lo < pl.hi <= F and pl.hi - pl.lo <= cf, label
            at = pl.hi
            # the warm-up: at most 64 frames, never before the start of the utterance that holds frame lo
            utt = max(s for s in starts if s <= pl.lo)
            assert pl.warm == min(pl.lo - utt, WARM) and pl.warm <= WARM and pl.lo - pl.warm >= utt, label
            # continues_prev: exactly when the chunk's first frame is not an utterance start
            assert bool(pl.continues_prev) == (pl.lo not in starts), label
            assert bool(pl.continues_next) == (pl.hi < F and pl.hi not in starts), label
            # stop: where the utterance of frame lo ends inside the chunk, counted from frame lo - warm
            nxt = min([s for s in starts if s > pl.lo] + [F])
            assert pl.stop == min(nxt, pl.hi) - (pl.lo - pl.warm), label
            # the upload: exactly the samples of frames [lo - warm, hi), inside the recording
            first = pl.lo - pl.warm
            assert s0 == first * H and s1 == (pl.hi - 1) * H + N and 0 <= s0 < s1 <= n_samples, label
            if c + 1 < len(plans):
                assert plans[c + 1][0].continues_prev == pl.continues_next, label
        assert at == F
        assert plans[0][0].continues_prev == 0 and plans[0][0].warm == 0 and plans[-1][0].continues_next == 0


def test_a_short_warm_up_still_continues(pkg):
    """An utterance that starts 10 frames before a cut: the warm-up is those 10 frames, and the cut is still one inside an utterance."""
    pl, s0, s1 = pkg.host_chunk_plan(650, 200, 2, N, H, np.array([0, 150, 200, 390, 600], dtype=np.int64))
    assert (pl.lo, pl.hi, pl.warm, pl.continues_prev) == (400, 600, 10, 1)
    assert pl.stop == 210 and pl.continues_next == 0          # the utterance ends where the chunk does: the next starts on the cut
    assert (s0, s1) == (390 * H, 599 * H + N)
    pl, _, _ = pkg.host_chunk_plan(650, 200, 1, N, H, np.array([0, 150, 200, 390, 600], dtype=np.int64))
    assert (pl.lo, pl.warm, pl.continues_prev, pl.stop, pl.continues_next) == (200, 0, 0, 190, 1)


def test_bad_arguments(pkg):
    with pytest.raises(pkg.VoxBoxError):
        pkg.host_chunk_plan(650, 200, 4, N, H)               # chunks 0..3 only
    with pytest.raises(pkg.VoxBoxError):
        pkg.host_chunk_plan(650, 0, 0, N, H)
    with pytest.raises(pkg.VoxBoxError):
        pkg.host_chunk_plan(650, 200, 0, N, 0)
    with pytest.raises(pkg.VoxBoxError):
        pkg.host_chunk_plan(650, 200, 0, N, H, np.array([1, 5], dtype=np.int64))
    with pytest.raises(pkg.VoxBoxError):
        pkg.host_chunk_plan(650, 200, 0, N, H, np.array([0, 9, 5], dtype=np.int64))
