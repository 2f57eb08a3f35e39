"""The pitch path's shard hand-off as arithmetic, without a GPU: the protocol of tests/pitch_path_shard_model.py (scan from a
guess, bit compare, repair, back map, end-state composition; shard.stitch_path drives it) gives the sequential model's path of the
whole recording for every world size -- on random lists and on the two streams whose unstitched contour is wrong on a third to a
half of the recording -- and shard.path_handoff moves the same states over a gloo group."""
import os
import socket
import sys

import numpy as np
import pytest

import pitch_path_model as M
import pitch_path_shard_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 3000
SEG = [0, 1100, 1130, 2000]


def _random_lists(rng, F, kmax, zero_frac=0.1):               # as tests/test_gpu_pitch_path.py
    f = rng.uniform(60.0, 650.0, (F, kmax))
    f[rng.uniform(size=(F, kmax)) < zero_frac] = 0.0
    a = rng.uniform(0.0, 1.0, (F, kmax))
    cand = np.stack([f, a], axis=-1)
    count = rng.integers(0, kmax + 3, F).astype(np.int32)
    status = np.where(rng.uniform(size=F) < 0.03, rng.integers(1, 5, F), 0).astype(np.int32)
    lp = rng.uniform(0.0, 1.0, F) ** 3
    return cand, count, status, lp


def _whole(cand, count, status, lp, seg, params):
    return M.path_states(M.frame_table(cand, count, status, lp, seg, params), seg)


_LISTS = {}


def _lists(kmax):
    if kmax not in _LISTS:
        _LISTS[kmax] = _random_lists(np.random.default_rng(2000 + kmax), F, kmax)
    return _LISTS[kmax]


@pytest.mark.parametrize("seg", [None, SEG], ids=["one_utterance", "four_utterances"])
@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("kmax", [1, 3, 15, 63])
def test_random_lists_shard_to_the_whole_path(pkg, kmax, world, seg):
    cand, count, status, lp = _lists(kmax)
    seg_a = None if seg is None else np.array(seg, np.int64)
    want = _whole(cand, count, status, lp, seg_a, M.DEFAULTS)
    got, redone, _ = S.run(pkg.shard, cand, count, status, lp, seg_a, M.DEFAULTS, world)
    assert np.array_equal(got, want)


def _unstitched(shard, cand, count, params, world):
    """Today's contour: every rank the path of the frames it analysed."""
    rows = []
    for r in range(world):
        pl = shard.plan(F, world, r, None)
        a = pl["lo"] - pl["warm"]
        tab = M.frame_table(cand[a:pl["hi"]], count[a:pl["hi"]], None, None, None, params)
        rows.append(M.path_states(tab, None)[pl["warm"]:])
    return np.concatenate(rows)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["late", "early"])
def test_the_two_streams(pkg, name, world):
    params = dict(M.DEFAULTS, **S.STREAM_PARAMS)
    cand, count = S.stream(name, world, F)
    want = _whole(cand, count, None, None, None, params)
    assert np.all(want == 1)                                   # the whole path is track 1 throughout
    loose = _unstitched(pkg.shard, cand, count, params, world)
    assert int(np.sum(loose != want)) == {2: 1500, 3: 1000}[world]
    got, redone, ranks = S.run(pkg.shard, cand, count, None, None, None, params, world)
    assert np.array_equal(got, want)
    if name == "late":                                         # every receiving rank's guess is wrong
        assert all(n > 0 for n in redone[1:]) and redone[0] == 0
    else:                                                      # rank 0's own leader is track 0
        last = ranks[0]
        assert int(M.leader(last.D[-1:], last.tab["active"][-1:])[0]) == 0


def test_end_states_compose_backwards(pkg):
    sh = pkg.shard
    plans = [dict(continues_prev=0, continues_next=1), dict(continues_prev=1, continues_next=1),
             dict(continues_prev=1, continues_next=0), dict(continues_prev=0, continues_next=0)]
    ident, swap, const = np.arange(64, dtype=np.int32), np.arange(64, dtype=np.int32), np.full(64, 5, np.int32)
    swap[[0, 1]] = [1, 0]
    assert sh.path_end_states([None, swap, const, None], plans) == [5, 5, None, None]
    assert sh.path_end_states([None, swap, np.full(64, 1, np.int32), None], plans) == [0, 1, None, None]
    assert sh.path_end_states([None, ident, np.full(64, 1, np.int32), None], plans) == [1, 1, None, None]
    assert sh.path_end_states([None], [dict(continues_prev=0, continues_next=0)]) == [None]


# ---- shard.path_handoff over gloo, world 3, the model standing in for the kernels ------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _handoff_worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    import pitch_path_model as M
    import pitch_path_shard_model as S
    sh = g.load_package().shard
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    params = dict(M.DEFAULTS, **S.STREAM_PARAMS)
    cand, count = S.stream("late", world, 3000)
    pl = sh.plan(3000, world, rank, None)
    a, b = pl["lo"] - pl["warm"], pl["hi"]
    tab = M.frame_table(cand[a:b], count[a:b], None, None, None, params)          # this rank's frames only
    rk = S.Rank(tab, None, pl["warm"], pl["continues_prev"], pl["continues_next"])
    redone = []

    def enter(state_in):
        so, bm, n = rk.enter(None if state_in is None else state_in.numpy())
        redone.append(n)
        return torch.from_numpy(so), torch.from_numpy(bm)

    end = sh.path_handoff(enter, pl)
    states = rk.finish(None if end is None else int(end.item()))
    np.save(os.path.join(out_dir, f"states_{rank}.npy"), states)
    np.save(os.path.join(out_dir, f"redone_{rank}.npy"), np.array(redone))
    dist.barrier()
    dist.destroy_process_group()


def test_path_handoff_over_gloo_at_world_3(tmp_path, pkg):
    import torch.multiprocessing as mp
    world = 3
    mp.start_processes(_handoff_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    params = dict(M.DEFAULTS, **S.STREAM_PARAMS)
    cand, count = S.stream("late", world, F)
    want = _whole(cand, count, None, None, None, params)
    got = np.concatenate([np.load(str(tmp_path / f"states_{r}.npy")) for r in range(world)])
    assert np.array_equal(got, want)
    redone = [int(np.load(str(tmp_path / f"redone_{r}.npy"))[0]) for r in range(world)]
    assert redone[0] == 0 and redone[1] > 0 and redone[2] > 0
