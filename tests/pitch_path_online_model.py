"""The online pitch path's definition (include/voxbox_hip.h "The pitch path while the lists arrive") as a
sequential numpy model, on top of pitch_path_model.frame_table / step: the oracle of vbx_path_stream_push.

The recursion is the resident path's.  What is new is WHEN a frame's state is known: after T frames of an utterance, decided(T) is
the length of the longest prefix on which the psi traces from all active states of frame T - 1 agree.  The model evaluates the
decisions after every frame (the schedule of one-frame pushes); the definition makes every other schedule commit the same states
with the same flags, and as many of them after the last frame of a push."""
import numpy as np

import pitch_path_model as M


def online_table(cand, count, status=None, local_peak=None, peak_ref=None, params=None):
    """frame_table with P = peak_ref for every frame: u_t of the online path (silence 0 or no peaks: u_t = voicing_threshold)."""
    tab = M.frame_table(cand, count, status, None, None, params)
    k = tab["k"]
    if local_peak is not None and k["silence"] != 0.0:
        lp = np.asarray(local_peak, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.zeros(tab["F"]) if peak_ref == 0.0 else lp / peak_ref
            v = 2.0 - rho / k["q"]
        u = k["vt"] + np.where(v > 0.0, v, 0.0)
        tab["u"] = u
        tab["lam"] = np.where(tab["voiced"], tab["lam"], u[:, None])
    return tab


def _row(tab, t):
    return {n: tab[n][t:t + 1] for n in ("lf", "voiced", "active", "lam")}


def run(tab, max_pending, marks=()):
    """The online path over all frames of tab.  marks: frame numbers t at which an utterance ends BEFORE frame t (an
    end_utterance flag behind frame t - 1; F = a flush at the end).  Returns a dict:
       states [F], forced [F] (bool)   what was committed for every frame (-1: never committed)
       committed [F + 1]               committed[T]: frames committed once T frames are pushed (marks at T applied)
       max_pending_seen                the largest number of frames held after a frame's decisions"""
    F, K = tab["F"], tab["K"]
    marks = set(int(m) for m in marks)
    states = np.full(F, -1, np.int64)
    forced = np.zeros(F, bool)
    committed = np.zeros(F + 1, np.int64)
    before_mark = np.zeros(F + 1, np.int64)                    # committed[T] before a mark at T is applied
    psi = np.zeros((F, K), np.int64)
    D, prev = None, None
    com = 0                                                    # frames committed (all utterances)
    seen = 0

    def walk(t_from, st, t_to):
        """the trace from state st at frame t_from down to frame t_to: {t: state}"""
        out = {}
        for t in range(t_from, t_to - 1, -1):
            out[t] = st
            st = int(psi[t, st])
        return out

    def decide(T):
        """commit what the traces from frame T - 1 agree on"""
        nonlocal com
        if T == com:
            return
        cur = np.flatnonzero(prev["active"][0])
        t = T - 1
        while t >= com:
            if np.all(cur == cur[0]):
                for tt, st in walk(t, int(cur[0]), com).items():
                    states[tt] = st
                com = t + 1
                return
            cur = psi[t, cur]
            t -= 1

    def leader_trace(T, t_hi, flag):
        """commit frames [com, t_hi] along the trace from the leader of frame T - 1"""
        nonlocal com
        st = int(M.leader(D, prev["active"])[0])
        tr = walk(T - 1, st, com)
        for tt in range(com, t_hi + 1):
            states[tt] = tr[tt]
            forced[tt] = flag
        com = t_hi + 1

    for t in range(F):
        before_mark[t] = com
        if t in marks:                                         # the utterance ends behind frame t - 1
            if t > com:
                leader_trace(t, t - 1, False)
            D, prev = None, None
            committed[t] = com
        if t - com == max_pending:                             # the ring is full (what is decided is committed already)
            leader_trace(t, com + (max_pending + 1) // 2 - 1, True)
        cur = _row(tab, t)
        D, p = M.step(D, prev, cur, tab["k"])
        psi[t] = p[0]
        prev = cur
        decide(t + 1)
        committed[t + 1] = com
        seen = max(seen, t + 1 - com)
    before_mark[F] = com
    if F in marks and F > com:
        leader_trace(F, F - 1, False)
        committed[F] = com
    return dict(states=states, forced=forced, committed=committed, before_mark=before_mark, max_pending_seen=seen)


def commits(res, pushes):
    """The vbx_path_commit of every push.  pushes: [(T, end)] -- the frames pushed once the push is through (ascending; a repeat
    is a zero-frame push) and its end_utterance flag (only at frames that run() got as marks).  [(first, n, n_forced, pending)]"""
    out = []
    com = 0
    marked = -1
    for T, end in pushes:
        if end:
            marked = T
        c = int(res["committed"][T] if marked == T else res["before_mark"][T])
        out.append((com, c - com, int(np.sum(res["forced"][com:c])), T - c))
        com = c
    return out
