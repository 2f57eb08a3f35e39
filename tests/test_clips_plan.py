"""vbx_clips_plan, the host arithmetic of vbx_analyze_clips, without a GPU: against a brute-force numpy restatement of the header's
rules, over hand-picked length lists (empty, all clips too short, N - 1 / N / N + 1, lengths = 0 and = 1 modulo the stride, a clip
larger than a group, stride > frame_len) and a few hundred lists from a fixed seed.  The invariants: rows are prefix sums of
vbx_frame_count, planes do not overlap, each clip's last real frame ends inside its own samples, every group holds whole clips in
order, the groups cover all clips with frames exactly once, and the invalid arguments are refused.  Frames longer than 4096 samples:
every clip is a group by itself."""
import ctypes as C

import numpy as np
import pytest

SHAPES = [(1200, 480), (1024, 512), (512, 512), (400, 1000), (7, 3), (1, 1), (4100, 2050)]
MAX_FRAME_LEN = 4096                   # longer frames: every clip is a group by itself (the header says why)


def default_group_frames(stride):
    """the header's default: the largest count whose f64 plane stays within VBX_CLIPS_PLANE_BYTES, in [64, 250000]"""
    return min(max((1 << 28) // 8 // stride, 64), 250000)


def brute_plan(lengths, N, H, group_frames):
    """the header's rules, clip by clip: (rows [n, 4], total, groups)"""
    gf = group_frames if group_frames else default_group_frames(H)
    rows, row, groups, nxt = [], 0, 0, 0
    for ln in lengths:
        n = 0 if ln < N else (ln - N) // H + 1
        if n == 0:
            rows.append((row, 0, -1, 0))
            continue
        if groups == 0 or N > MAX_FRAME_LEN or nxt + n > gf:                                  # the clip would take the open group past gf frames
            groups, nxt = groups + 1, 0
        rows.append((row, n, groups - 1, nxt))
        nxt += -(-ln // H)
        row += n
    return np.array(rows, np.int64).reshape(len(lengths), 4), row, groups


def check_invariants(pkg, lengths, N, H, gf, rows, total, groups):
    lengths = [int(v) for v in lengths]
    counts = [pkg.frame_count(ln, N, H) for ln in lengths]
    assert list(rows[:, 1]) == counts and total == sum(counts)
    assert list(rows[:, 0]) == [sum(counts[:b]) for b in range(len(lengths))]                # prefix sums
    live = [b for b in range(len(lengths)) if counts[b]]
    assert all(rows[b, 2] == -1 and rows[b, 3] == 0 for b in range(len(lengths)) if not counts[b])
    # the groups cover the clips with frames exactly once, in order, as runs of whole clips
    g_of = [int(rows[b, 2]) for b in live]
    assert g_of == sorted(g_of) and (not live or (g_of[0] == 0 and g_of[-1] == groups - 1)) and len(set(g_of)) == groups
    eff = gf if gf else default_group_frames(H)
    for g in range(groups):
        mem = [b for b in live if rows[b, 2] == g]
        assert mem and rows[mem[0], 3] == 0
        for a, b in zip(mem, mem[1:]):
            # planes do not overlap: clip b starts at or behind clip a's end, less than one hop behind it
            end_a = int(rows[a, 3]) * H + lengths[a]
            assert end_a <= int(rows[b, 3]) * H < end_a + H
        for b in mem:
            # the clip's last real frame ends inside its own samples (the plane element of its sample 0 is plane_frame * H)
            assert (int(rows[b, 1]) - 1) * H + N <= lengths[b]
        frames = int(rows[mem[-1], 3] + rows[mem[-1], 1])
        assert frames <= eff or len(mem) == 1                                                 # a clip larger on its own: a group by itself
        if N > MAX_FRAME_LEN:
            assert len(mem) == 1
        elif g + 1 < groups:                                                                  # greedy: the next clip did not fit any more
            nb = [b for b in live if rows[b, 2] == g + 1][0]
            nxt = int(rows[mem[-1], 3]) + -(-lengths[mem[-1]] // H)
            assert nxt + counts[nb] > eff


def hand_lists(N, H):
    big = N + 64 * H + 5
    return [[], [0], [N - 1], [0, 1, N - 1], [N], [N - 1, N, N + 1], [N + H - 1, N + H, N + H + 1],
            [3 * H, 3 * H + 1, N + 2 * H, N + 2 * H + 1] if 3 * H >= N else [N + 3 * H, N + 3 * H + 1],
            [-(-N // H) * H, -(-N // H) * H + 1, N], [N, 0, N, N - 1, N], [big, N, big, N, N], [N] * 70, [N, big * 3, N],
            [N + 299 * H, N, 0, N + 1]]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}/{h}" for n, h in SHAPES])
def test_the_plan_is_the_brute_force_plan(pkg, shape):
    N, H = shape
    rng = np.random.default_rng(20260 + N + H)
    lists = hand_lists(N, H)
    for _ in range(60):                                                                       # 420 random lists over the seven shapes
        n = int(rng.integers(1, 40))
        kind = rng.integers(0, 3)
        if kind == 0:
            ls = rng.integers(0, N + 6 * H, n)
        elif kind == 1:
            ls = N + H * rng.integers(0, 90, n) + rng.integers(-1, 2, n)                      # around the frame boundaries
        else:
            ls = np.where(rng.random(n) < 0.3, rng.integers(0, N, n), N + rng.integers(0, 200 * H, n))
        lists.append([int(v) for v in ls])
    seen = dict(single=False, many=False, short=False, cut=False)
    for ls in lists:
        for gf in (0, 64, 65, 100, 4096):
            rows, total, groups = pkg.clips_plan(ls, N, H, gf)
            want = brute_plan(ls, N, H, gf)
            assert np.array_equal(rows, want[0]) and (total, groups) == want[1:], (ls, gf)
            check_invariants(pkg, ls, N, H, gf, rows, total, groups)
            seen["single"] |= any(r[1] > gf for r in rows) and gf != 0
            seen["many"] |= groups > 2
            seen["short"] |= any(r[2] == -1 for r in rows)
            seen["cut"] |= groups > 1 and gf != 0
    assert all(seen.values()), seen
    assert pkg.clips_plan([], N, H)[1:] == (0, 0)
    assert pkg.clips_plan([N - 1, 0], N, H)[1:] == (0, 0)


def test_the_default_group_keeps_an_f64_plane_within_the_stated_bytes(pkg):
    for H in (1, 160, 480, 512, 2050, 1 << 20, 1 << 30):
        gf = default_group_frames(H)
        N = min(max(H // 2, 1), MAX_FRAME_LEN)
        ls = [N + (gf - 1) * H, N]                                                            # exactly gf frames, then one more
        rows, total, groups = pkg.clips_plan(ls, N, H, 0)
        assert groups == 2 and total == gf + 1, H
        assert groups == 2 and pkg.clips_plan([N + (gf - 2) * H, N], N, H, 0)[2] == 1
        assert 64 <= gf <= 250000 and (gf * H * 8 <= pkg.CLIPS_PLANE_BYTES or gf == 64)


def test_bad_arguments(pkg):
    L = pkg.load_library()
    sz = C.c_size_t
    ln = (sz * 3)(1200, 5000, 0)
    rows = (pkg.ClipRow * 3)()
    total, groups = sz(7), sz(7)
    assert L.vbx_clips_plan(ln, 3, 1200, 480, 0, rows, C.byref(total), C.byref(groups)) == 0
    assert (total.value, groups.value) == (1 + 8, 1)
    assert L.vbx_clips_plan(ln, 3, 1200, 480, 64, rows, None, None) == 0                      # the totals are optional
    assert L.vbx_clips_plan(None, 0, 1200, 480, 0, None, C.byref(total), C.byref(groups)) == 0 and (total.value, groups.value) == (0, 0)
    for bad in ((None, 3, 1200, 480, 0, rows), (ln, 3, 1200, 480, 0, None), (ln, 3, 0, 480, 0, rows), (ln, 3, 1200, 0, 0, rows),
                (ln, 3, 1200, 480, 1, rows), (ln, 3, 1200, 480, 63, rows)):
        assert L.vbx_clips_plan(*bad, C.byref(total), C.byref(groups)) == -1, bad
    # more than 0x7fffffff rows, in one clip and in the sum
    huge = (sz * 2)(1 << 31, 1)
    assert L.vbx_clips_plan(huge, 2, 1, 1, 0, rows, None, None) == -1
    half = (sz * 3)(1 << 30, 1 << 30, 1)
    assert L.vbx_clips_plan(half, 3, 2, 1, 0, rows, C.byref(total), None) == 0 and total.value == (1 << 31) - 2
    assert L.vbx_clips_plan((sz * 3)(1 << 30, 1 << 30, 3), 3, 2, 1, 0, rows, None, None) == -1
    with pytest.raises(pkg.VoxBoxError):
        pkg.clips_plan([1200], 1200, 480, 5)
