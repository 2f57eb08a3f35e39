"""Frame-range sharding of one long recording across the GPUs of a node.

Frames are independent on the whole path except for the formant tracker, whose state is
reset at utterance boundaries, so the batch splits by contiguous frame ranges with no
data-path collective; the only exchange is one gather of fixed-size per-frame records to
rank 0 (RCCL over xGMI when the tensors live on the GPUs, gloo in the CPU tests).  Two sequential steps cross a cut inside
an utterance: the formant tracker's state (plan, stitch_rows) and the pitch path's (path_end_states, stitch_path, path_handoff).
"""
import numpy as np


def frame_range(rank, world, n_frames):
    """Contiguous split [lo, hi) of n_frames over `world` ranks (first ranks take the remainder)."""
    base, rem = divmod(n_frames, world)
    lo = rank * base + min(rank, rem)
    hi = lo + base + (1 if rank < rem else 0)
    return lo, hi


def segment_aligned_ranges(world, seg_start, n_frames):
    """Split at utterance boundaries so every tracker segment lives on exactly one rank.
    seg_start: ascending frame indices (seg_start[0] == 0).  Returns [(lo, hi)] per rank."""
    seg = np.asarray(seg_start, dtype=np.int64)
    bounds = np.append(seg, n_frames)
    out = []
    prev = 0
    for r in range(world):
        target = frame_range(r, world, n_frames)[1]
        # first boundary >= target (the last rank always ends at n_frames)
        idx = int(np.searchsorted(bounds, target, side="left"))
        hi = int(bounds[min(idx, len(bounds) - 1)]) if r < world - 1 else n_frames
        hi = max(hi, prev)
        out.append((prev, hi))
        prev = hi
    return out


WARM_FRAMES = 64          # == VBX_SHARD_WARM_FRAMES


def shard_ranges(world, seg_start, n_frames):
    """vbx_shard_range for every rank: the even split; a cut moves up to an utterance start that lies within 1/32 of a
    shard after it, otherwise it stays where it is -- inside the utterance (the track is carried across, `plan`)."""
    bounds = None if seg_start is None else np.asarray(seg_start, dtype=np.int64)
    slack = n_frames // world // 32
    cuts = [0]
    for r in range(world):
        if r == world - 1:
            c = n_frames
        else:
            c = frame_range(r, world, n_frames)[1]
            if bounds is not None and bounds.size:
                idx = int(np.searchsorted(bounds, c, side="left"))
                if idx < bounds.size and bounds[idx] <= c + slack and bounds[idx] <= n_frames:
                    c = int(bounds[idx])
        cuts.append(max(c, cuts[-1]))
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def plan(n_frames, world, rank, seg_start=None, warm_frames=WARM_FRAMES):
    """vbx_shard_plan as a dict: lo, hi, warm (extra leading frames [lo - warm, lo) that warm the tracker up), stop (index
    from frame lo - warm at which the utterance holding frame lo ends inside the shard), continues_prev / continues_next."""
    seg = np.array([0], dtype=np.int64) if seg_start is None else np.asarray(seg_start, dtype=np.int64)
    lo, hi = shard_ranges(world, seg_start, n_frames)[rank]
    start_of = lambda f: int(seg[np.searchsorted(seg, f, side="right") - 1]) if seg.size else 0
    continued = lambda c: 0 < c < n_frames and c - start_of(c) > warm_frames
    out = dict(lo=lo, hi=hi, warm=0, stop=0, continues_prev=0, continues_next=0)
    if hi <= lo:
        return out
    out["warm"] = min(lo - start_of(lo), warm_frames)
    out["continues_prev"] = int(continued(lo))
    out["continues_next"] = int(continued(hi))
    after = seg[seg > lo]
    nxt = min(int(after[0]), n_frames) if after.size else n_frames
    out["stop"] = min(nxt, hi) - (lo - out["warm"])
    return out


def plan_local_segments(pl, seg_start=None):
    """vbx_shard_local_segments: utterance starts of frames [lo - warm, hi), re-based (first entry 0)."""
    first = pl["lo"] - pl["warm"]
    if seg_start is None:
        return np.array([0], dtype=np.int64)
    seg = np.asarray(seg_start, dtype=np.int64)
    return np.concatenate([[0], seg[(seg > first) & (seg < pl["hi"])] - first]).astype(np.int64)


def stitch_rows(rows, first, stop, state_in, step):
    """The repair step of vbx_track_stitch_f64 on host arrays (the CPU tests' stand-in for the kernel; `step(state, t)` is
    one tracker step on local frame t and returns the new state).  rows: [n, n_est, 2] formant rows of frames
    [lo - warm, hi) tracked from a guess; state_in: the row the previous rank ends with.  Rows [first, stop) are rewritten
    until the redone scan meets a row it already holds.  Returns the number of rows rewritten."""
    state = np.array(state_in, dtype=np.float64, copy=True)
    if first > 0 and rows[first - 1].tobytes() == state.tobytes():
        return 0
    n = 0
    for t in range(first, stop):
        state = step(state, t)
        if rows[t].tobytes() == state.tobytes():
            break
        rows[t] = state
        n += 1
    return n


def sample_range(lo, hi, frame_len, hop):
    """Samples [s0, s1) a rank needs for frames [lo, hi): includes the (frame_len - hop) halo."""
    if hi <= lo:
        return lo * hop, lo * hop
    return lo * hop, (hi - 1) * hop + frame_len


def local_segments(seg_start, lo, hi):
    """Tracker segment starts of the frames [lo, hi), re-based to the shard (first entry 0)."""
    seg = np.asarray(seg_start, dtype=np.int64)
    inside = seg[(seg > lo) & (seg < hi)] - lo
    return np.concatenate([[0], inside]).astype(np.int64)


def gather_records(local, counts, dst=0, group=None):
    """Gathers per-frame record tensors [n_local, rec] from every rank to `dst` in rank order.
    `counts[r]` = frames owned by rank r.  Uses torch.distributed (nccl == RCCL on ROCm, or
    gloo).  Returns the concatenated [sum(counts), rec] tensor on dst, None elsewhere."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    rec = local.shape[1:]
    if world == 1:
        return local
    if dist.get_backend(group) == "nccl":
        # one grouped send/recv set: every peer's payload crosses its own xGMI link to dst
        if rank == dst:
            parts = [local if r == dst else torch.empty((counts[r],) + tuple(rec), dtype=local.dtype, device=local.device)
                     for r in range(world)]
            ops = [dist.P2POp(dist.irecv, parts[r], r, group) for r in range(world) if r != dst and counts[r] > 0]
            if ops:
                for w in dist.batch_isend_irecv(ops):
                    w.wait()
            return torch.cat(parts, dim=0)
        if counts[rank] > 0:
            for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, local.contiguous(), dst, group)]):
                w.wait()
        return None
    # gloo (CPU tests): pad to the largest shard and use gather
    mx = max(counts)
    pad = torch.zeros((mx,) + tuple(rec), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    if rank == dst:
        bufs = [torch.empty_like(pad) for _ in range(world)]
        dist.gather(pad, bufs, dst=dst, group=group)
        return torch.cat([bufs[r][: counts[r]] for r in range(world)], dim=0)
    dist.gather(pad, None, dst=dst, group=group)
    return None


# ---- the pitch path across shard cuts (include/voxbox_hip.h, "The pitch path across a shard cut") ----------------------------

PATH_STATES = 64          # == VBX_PITCH_PATH_STATES


def _plan_flag(pl, name):
    return bool(pl[name] if isinstance(pl, dict) else getattr(pl, name))


def path_end_states(back_maps, plans):
    """Step 3 of the protocol on the host: the state of every rank's last frame on the whole recording's path, from the last
    rank backwards -- end[r] = back_map[r + 1][end[r + 1]] wherever rank r continues into rank r + 1, None elsewhere (that
    rank's last utterance ends at its own leader).  back_maps[r]: the 64 int32 vbx_pitch_path_shard_enter_f64 wrote on rank
    r (None where rank r does not continue its predecessor); plans[r]: vbx_shard_plan of rank r (dict or ShardPlan).  Where
    rank r + 1's utterance ends inside its shard its back map is constant: entry 0 is read."""
    world = len(plans)
    end = [None] * world
    for r in range(world - 2, -1, -1):
        if _plan_flag(plans[r], "continues_next"):
            e = end[r + 1] if end[r + 1] is not None else 0
            end[r] = int(back_maps[r + 1][e])
    return end


def stitch_path(enter, finish, plans):
    """The protocol after every rank's begin, on one host (the counterpart of stitch_rows: the CPU tests pass the numpy model's
    steps, a single-device run the VoxBox calls of one context per rank).  enter(r, state_in) -> (state_out [64] f64,
    back_map [64] int32, chunks_redone) runs in rank order, state_in = rank r - 1's state_out when rank r continues it, else
    None; finish(r, end_state) -> that rank's rows, end_state None where the rank does not continue into the next.
    Returns ([rows of rank 0, rows of rank 1, ..], [chunks_redone per rank])."""
    world = len(plans)
    state, maps, changed = None, [], []
    for r in range(world):
        state, bm, n = enter(r, state if _plan_flag(plans[r], "continues_prev") else None)
        maps.append(bm)
        changed.append(int(n))
    end = path_end_states(maps, plans)
    return [finish(r, end[r]) for r in range(world)], changed


def path_handoff(enter, plan, group=None, device=None):
    """One rank's part of the protocol over a torch.distributed group (any backend with send / recv: gloo in the CPU test).
    The states travel forward along the chain of ranks, the end states backward:
      receive 64 doubles from rank - 1 when plan.continues_prev; enter(state_in or None) -> (state_out, back_map), tensors of
      64 float64 / 64 int32 on `device` (what the backend moves: None = the CPU, for gloo); send state_out to rank + 1 when
      plan.continues_next;
      receive this rank's end state (one int32) from rank + 1 when plan.continues_next; send back_map[end state, or 0 when
      the utterance ends here] to rank - 1 when plan.continues_prev.
    Returns the end state for vbx_pitch_path_shard_finish_f64 as a one-element int32 tensor like back_map, or None."""
    import torch
    import torch.distributed as dist
    rank = dist.get_rank(group)
    prev, nxt = _plan_flag(plan, "continues_prev"), _plan_flag(plan, "continues_next")
    state_in = None
    if prev:
        state_in = torch.empty(PATH_STATES, dtype=torch.float64, device=device)
        dist.recv(state_in, src=rank - 1, group=group)
    state_out, back_map = enter(state_in)
    if nxt:
        dist.send(state_out.contiguous(), dst=rank + 1, group=group)
    end = None
    if nxt:
        end = torch.empty(1, dtype=torch.int32, device=device)
        dist.recv(end, src=rank + 1, group=group)
    if prev:
        e = int(end.item()) if end is not None else 0
        dist.send(back_map[e:e + 1].to(torch.int32).contiguous(), dst=rank - 1, group=group)
    return end
