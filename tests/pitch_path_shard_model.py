"""The pitch path's shard hand-off (include/voxbox_hip.h, "The pitch path across a shard cut") in numpy, on top of the
sequential model of tests/pitch_path_model.py: one Rank per shard does what vbx_pitch_path_shard_begin_f64 / _enter / _finish
do -- scan the local frames from a guess, compare the received state bit for bit, repair, back map, end state -- and
run() drives the protocol through shard.stitch_path.  Also the test streams of the hand-off's tests (CPU and GPU)."""
import numpy as np

import pitch_path_model as M

STATES = 64               # VBX_PITCH_PATH_STATES


def _row(tab, t):
    return {n: tab[n][t:t + 1] for n in ("lf", "voiced", "active", "lam")}


def _pad(D):
    out = np.full(STATES, -np.inf)
    out[:D.size] = D
    return out


class Rank:
    """One rank: local frames [0, n) = global frames [lo - warm, hi); first = warm.  tab: M.frame_table of the LOCAL frames (with
    the utterance's whole P in u_t when the silence term is on); seg_start: the local utterance starts."""

    def __init__(self, tab, seg_start, first, continues_prev, continues_next):
        self.tab, self.first, self.prev, self.next = tab, int(first), bool(continues_prev), bool(continues_next)
        self.n, self.K = tab["F"], tab["K"]
        self.segs = [(s0, s1) for s0, s1 in M.segments(seg_start, self.n) if s1 > s0]
        self.D = np.full((self.n, self.K), -np.inf)
        self.psi = np.zeros((self.n, self.K), np.int64)
        for s0, s1 in self.segs:                                # begin: every local utterance from a fresh start
            self._scan(s0, s1, None)

    def _scan(self, t0, t1, D, stop_when_met=False):
        """Frames [t0, t1) from the state D of frame t0 - 1 (None: a fresh start).  Returns the frames rewritten."""
        n = 0
        for t in range(t0, t1):
            D, p = M.step(D, None if t == t0 and D is None else _row(self.tab, t - 1), _row(self.tab, t), self.tab["k"])
            if stop_when_met and self.D[t].tobytes() == D[0].tobytes() and np.array_equal(self.psi[t], p[0]):
                break
            self.D[t], self.psi[t] = D[0], p[0]
            n += 1
        return n

    def _segment_of(self, t):
        return next((s0, s1) for s0, s1 in self.segs if s0 <= t < s1)

    def enter(self, state_in):
        """(state_out [64], back_map [64] int32, frames redone)."""
        assert (state_in is not None) == self.prev
        redone = 0
        if self.prev and self.first < self.n:
            want = np.asarray(state_in, np.float64)[:self.K]
            if want.tobytes() != self.D[self.first - 1].tobytes():
                _, s1 = self._segment_of(self.first)
                redone = self._scan(self.first, s1, want[None, :], stop_when_met=True)
        if self.n == 0:
            return _pad(np.zeros(0)), np.zeros(STATES, np.int32), 0
        state_out = _pad(np.asarray(state_in, np.float64)[:self.K]) if (self.prev and self.first == self.n) else _pad(self.D[-1])
        # the end state of every local utterance but an open last one is its leader
        self.lead = {}
        for s0, s1 in self.segs:
            self.lead[s0] = int(M.leader(self.D[s1 - 1:s1], self.tab["active"][s1 - 1:s1])[0])
        back = np.zeros(STATES, np.int32)
        if self.first >= 1:
            s0, s1 = self._segment_of(self.first - 1)
            open_ = self.next and s1 == self.n
            for e in range(self.K if open_ else 1):
                st = e if open_ else self.lead[s0]
                for t in range(s1 - 1, self.first - 1, -1):
                    st = int(self.psi[t, st])
                back[e if open_ else slice(None)] = st
        return state_out, back, redone

    def finish(self, end_state):
        """The states of local frames [first, n)."""
        assert (end_state is not None) == self.next
        states = np.zeros(self.n, np.int64)
        for s0, s1 in self.segs:
            st = int(end_state) if (self.next and s1 == self.n) else self.lead[s0]
            for t in range(s1 - 1, s0 - 1, -1):
                states[t] = st
                st = int(self.psi[t, st])
        return states[self.first:]


def global_u(cand, count, status, local_peak, seg_start, params):
    """u_t of every frame of the whole recording (P per utterance of the WHOLE recording)."""
    return M.frame_table(cand, count, status, local_peak, seg_start, params)["u"]


def run(shard, cand, count, status, local_peak, seg_start, params, world, plans=None, lseg=None):
    """The sharded path of the whole recording: (states [F], frames redone per rank, ranks).  `shard`: the product's shard
    module (plan, plan_local_segments, stitch_path).  P is taken globally: every rank's u_t is the whole recording's."""
    F = np.asarray(cand).shape[0]
    u = global_u(cand, count, status, local_peak, seg_start, params)
    plans = plans if plans is not None else [shard.plan(F, world, r, seg_start) for r in range(world)]
    ranks = []
    for r, pl in enumerate(plans):
        a, b = pl["lo"] - pl["warm"], pl["hi"]
        ls = shard.plan_local_segments(pl, seg_start) if lseg is None else lseg[r]
        tab = M.frame_table(cand[a:b], count[a:b], None if status is None else status[a:b], None, ls, params)
        tab["u"] = u[a:b].copy()
        tab["lam"] = np.where(tab["voiced"], tab["lam"], tab["u"][:, None])
        ranks.append(Rank(tab, ls, pl["warm"], pl["continues_prev"], pl["continues_next"]))
    rows, redone = shard.stitch_path(lambda r, s: ranks[r].enter(s), lambda r, e: ranks[r].finish(e), plans)
    return np.concatenate(rows), redone, ranks


# ---- the two streams: _adversarial's tracks (tests/test_gpu_pitch_path.py) with a drift that changes sign at frame B ---------

def _tracks(d):
    F = d.size
    cand = np.zeros((F, 2, 2))
    cand[:, 0] = np.stack([np.full(F, 200.0), 0.7 + d / 2], axis=-1)
    cand[:, 1] = np.stack([np.full(F, 200.0 * 2 ** 0.5), 0.7 - d / 2 - 0.005], axis=-1)
    return cand, np.full(F, 2, np.int32)


def late_stream(F, B):
    """Track 1 leads before B, track 0 gains after it: a rank that starts fresh after B follows the wrong track (forward)."""
    rng = np.random.default_rng(5)
    d = np.where(np.arange(F) < B, -2e-4, 1e-4) + rng.uniform(-1e-5, 1e-5, F)
    return _tracks(d)


def early_stream(F, B):
    """Track 0 leads narrowly before B, track 1 gains after it: rank 0's own leader is not on the whole path (backward)."""
    rng = np.random.default_rng(6)
    d = np.where(np.arange(F) < B, 1e-5, -1e-4) + rng.uniform(-1e-6, 1e-6, F)
    return _tracks(d)


STREAM_PARAMS = dict(silence_threshold=0.0)
STREAM_B = {("late", 2): 1468, ("late", 3): 1968, ("early", 2): 1500, ("early", 3): 1000}


def stream(name, world, F=3000):
    return (late_stream if name == "late" else early_stream)(F, STREAM_B[(name, world)])
