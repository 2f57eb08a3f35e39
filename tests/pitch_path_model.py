"""The pitch path's definition (include/voxbox_hip.h, DESIGN.md "Pitch path") as a sequential numpy model: the oracle of
vbx_pitch_path_f64 (the crate has none -- PitchExtractor, src/periodic.rs:320-354, returns candidates[t][0]).

Every operation is the definition's, in its order, in IEEE binary64 (numpy does not fuse multiply-adds).  The model loops over
frames and vectorises across segments of equal length.  States of a frame live in K = kmax + 1 columns: the listed entries
first, the appended unvoiced state at column m (when there is one); inactive columns hold D = -inf."""
import numpy as np

# Praat's "To Pitch (ac)" defaults (time_step: a 10 ms hop)
DEFAULTS = dict(voicing_threshold=0.45, silence_threshold=0.03, octave_cost=0.01, octave_jump_cost=0.35,
                voiced_unvoiced_cost=0.14, ceiling_hz=600.0, time_step=0.01)


def constants(params):
    p = dict(DEFAULTS, **(params or {}))
    corr = 0.01 / p["time_step"]
    return dict(vt=p["voicing_threshold"], oc=p["octave_cost"], cvu=p["voiced_unvoiced_cost"] * corr,
                cj=p["octave_jump_cost"] * corr, Lc=np.log2(p["ceiling_hz"]),
                q=p["silence_threshold"] / (1.0 + p["voicing_threshold"]), silence=p["silence_threshold"])


def segments(seg_start, F):
    """[(s0, s1)] of every segment (empty ones included); None / empty = one segment."""
    if seg_start is None or len(seg_start) == 0:
        return [(0, F)]
    s = [int(v) for v in seg_start] + [F]
    return [(s[i], s[i + 1]) for i in range(len(s) - 1)]


def unvoiced_scores(F, local_peak, seg_start, k):
    """u_t of every frame."""
    u = np.full(F, k["vt"])
    if local_peak is None or k["silence"] == 0.0:
        return u
    lp = np.asarray(local_peak, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s0, s1 in segments(seg_start, F):
            if s1 <= s0:
                continue
            P = np.fmax.reduce(lp[s0:s1])                      # NaN entries ignored, as fmax on the device
            rho = np.zeros(s1 - s0) if P == 0.0 else lp[s0:s1] / P
            v = 2.0 - rho / k["q"]
            u[s0:s1] = k["vt"] + np.where(v > 0.0, v, 0.0)
    return u


def frame_table(cand, count, status, local_peak, seg_start, params):
    """Per frame: m (listed states), n (all states), u; per frame and state column: lam, lf, voiced, active."""
    cand = np.asarray(cand, dtype=np.float64)
    F, kmax = cand.shape[0], cand.shape[1]
    K = kmax + 1
    k = constants(params)
    ok = np.ones(F, bool) if status is None else (np.asarray(status) == 0)
    m = np.where(ok, np.clip(np.asarray(count, dtype=np.int64), 0, kmax), 0)
    col = np.arange(K)[None, :]
    f = np.zeros((F, K)); a = np.zeros((F, K))
    f[:, :kmax] = cand[:, :, 0]; a[:, :kmax] = cand[:, :, 1]
    listed = col < m[:, None]
    has_zero = np.any(listed & (f == 0.0), axis=1)
    n = m + (~has_zero).astype(np.int64)
    active = col < n[:, None]
    voiced = listed & (f > 0.0)
    lf = np.where(voiced, np.log2(np.where(voiced, f, 1.0)), 0.0)
    u = unvoiced_scores(F, local_peak, seg_start, k)
    lam = np.where(voiced, a - k["oc"] * (k["Lc"] - lf), u[:, None])
    return dict(F=F, K=K, kmax=kmax, m=m, n=n, u=u, lam=lam, lf=lf, voiced=voiced, active=active, cand=cand, k=k)


def transition_costs(prev_lf, prev_voiced, cur_lf, cur_voiced, k):
    """c(p -> s) for [S, K] previous / current columns: [S, Kp, Ks]."""
    vp = prev_voiced[:, :, None]; vs = cur_voiced[:, None, :]
    both = k["cj"] * np.abs(prev_lf[:, :, None] - cur_lf[:, None, :])
    return np.where(vp & vs, both, np.where(vp != vs, k["cvu"], 0.0))


def step(D_prev, prev, cur, k):
    """One frame of the recursion for S rows at once.  D_prev: [S, K] (None: the segment's first frame); prev / cur: dicts of
    [S, K] arrays lf, voiced, active, lam.  Returns (D [S, K], psi [S, K])."""
    S, K = cur["lam"].shape
    if D_prev is None:
        e = cur["lam"].copy()
        psi = np.zeros((S, K), np.int64)
    else:
        c = transition_costs(prev["lf"], prev["voiced"], cur["lf"], cur["voiced"], k)
        vals = np.where(prev["active"][:, :, None], D_prev[:, :, None] - c, -np.inf)
        psi = np.argmax(vals, axis=1)                          # the first maximum: ties go to the lower index
        e = np.take_along_axis(vals, psi[:, None, :], axis=1)[:, 0, :] + cur["lam"]
    e = np.where(cur["active"], e, -np.inf)
    mx = np.max(e, axis=1)
    D = np.where(cur["active"], e - mx[:, None], -np.inf)
    return D, np.where(cur["active"], psi, 0)


def leader(D, active):
    """The first state with D == 0 (0 if there is none)."""
    return np.argmax((D == 0.0) & active, axis=1)


def _rows(tab, idx):
    return {n: tab[n][idx] for n in ("lf", "voiced", "active", "lam")}


def path_states(tab, seg_start):
    """The chosen state (column) of every frame."""
    F, K = tab["F"], tab["K"]
    states = np.zeros(F, np.int64)
    by_len = {}
    for s0, s1 in segments(seg_start, F):
        if s1 > s0:
            by_len.setdefault(s1 - s0, []).append(s0)
    for L, starts in by_len.items():
        idx = np.asarray(starts, np.int64)[:, None] + np.arange(L)[None, :]
        S = idx.shape[0]
        psi = np.zeros((S, L, K), np.uint8)
        D, prev = None, None
        for t in range(L):
            cur = _rows(tab, idx[:, t])
            D, p = step(D, prev, cur, tab["k"])
            psi[:, t] = p
            prev = cur
        st = leader(D, prev["active"])
        states[idx[:, L - 1]] = st
        rows = np.arange(S)
        for t in range(L - 1, 0, -1):
            st = psi[rows, t, st].astype(np.int64)
            states[idx[:, t - 1]] = st
    return states


def outputs(tab, states):
    """(out_path [F, 2], out_index [F]) of a state sequence."""
    F = tab["F"]
    rows = np.arange(F)
    listed = states < tab["m"]
    voiced = tab["voiced"][rows, states]
    path = np.zeros((F, 2))
    ent = tab["cand"][rows, np.minimum(states, tab["kmax"] - 1)]
    path[:, 0] = np.where(voiced, ent[:, 0], 0.0)
    path[:, 1] = np.where(voiced, ent[:, 1], tab["u"])
    return path, np.where(listed, states, -1).astype(np.int32)


def pitch_path(cand, count, status=None, local_peak=None, seg_start=None, params=None):
    """The model of vbx_pitch_path_f64: (out_path [F, 2], out_index [F])."""
    tab = frame_table(cand, count, status, local_peak, seg_start, params)
    return outputs(tab, path_states(tab, seg_start))


def states_from_index(tab, index):
    """Columns back from out_index (-1 = the appended unvoiced state at column m)."""
    index = np.asarray(index, np.int64)
    return np.where(index >= 0, index, tab["m"])


def path_score(tab, states, s0, s1):
    """Total score of the state sequence over frames [s0, s1): sum lambda - sum c (float; the near-tie measure)."""
    t = np.arange(s0, s1)
    tot = float(np.sum(tab["lam"][t, states[t]]))
    if s1 - s0 > 1:
        p, s = states[t[:-1]], states[t[1:]]
        vp, vs = tab["voiced"][t[:-1], p], tab["voiced"][t[1:], s]
        lp, ls = tab["lf"][t[:-1], p], tab["lf"][t[1:], s]
        c = np.where(vp & vs, tab["k"]["cj"] * np.abs(lp - ls), np.where(vp != vs, tab["k"]["cvu"], 0.0))
        tot -= float(np.sum(c))
    return tot
