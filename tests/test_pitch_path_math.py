"""The pitch path's definition (tests/pitch_path_model.py) checked without a GPU: the normalised recursion finds the best path
of an exhaustive enumeration scored in exact rational arithmetic, its decisions are the running-sum recursion's, and its state
forgets its history after a frame with a dominant leader -- the property the device's chunked scan relies on."""
import itertools
from fractions import Fraction

import numpy as np

import pitch_path_model as M


def _random_case(rng, T, kmax=3):
    f = rng.uniform(70.0, 600.0, (T, kmax))
    f[rng.uniform(size=(T, kmax)) < 0.15] = 0.0
    cand = np.stack([f, rng.uniform(0.0, 1.0, (T, kmax))], axis=-1)
    count = rng.integers(0, kmax + 2, T).astype(np.int32)
    status = np.where(rng.uniform(size=T) < 0.1, 3, 0).astype(np.int32)
    lp = rng.uniform(0.0, 1.0, T)
    params = dict(M.DEFAULTS, octave_jump_cost=rng.uniform(0.0, 2.0), voiced_unvoiced_cost=rng.uniform(0.0, 1.0),
                  octave_cost=rng.uniform(0.0, 0.1))
    return cand, count, status, lp, params


def _cost(tab, t, p, s):
    """c(p -> s) into frame t, as the float the definition computes."""
    row = lambda n, i, j: tab[n][i:i + 1, j:j + 1]
    return float(M.transition_costs(row("lf", t - 1, p), row("voiced", t - 1, p), row("lf", t, s), row("voiced", t, s), tab["k"])[0, 0, 0])


def _exact_score(tab, states):
    tot = Fraction(0)
    for t, s in enumerate(states):
        tot += Fraction(float(tab["lam"][t, s]))
        if t:
            tot -= Fraction(_cost(tab, t, states[t - 1], s))
    return tot


def test_the_path_attains_the_exhaustive_maximum():
    rng = np.random.default_rng(2024)
    n_cases = 0
    for _ in range(300):
        T = int(rng.integers(1, 8))
        cand, count, status, lp, params = _random_case(rng, T)
        tab = M.frame_table(cand, count, status, lp, None, params)
        choices = [range(int(n)) for n in tab["n"]]
        if np.prod([len(c) for c in choices]) > 5000:
            continue
        scores = {seq: _exact_score(tab, seq) for seq in itertools.product(*choices)}
        best = max(scores.values())
        got = tuple(int(s) for s in M.path_states(tab, None))
        assert got in scores
        assert scores[got] == best or best - scores[got] <= Fraction(1, 10**12), (got, float(best - scores[got]))
        n_cases += 1
    assert n_cases > 250


def _running_sum_psi(tab):
    """The textbook recursion: delta_t(s) = max_p (delta_{t-1}(p) - c) + lambda, no normalisation; psi and its margins."""
    T, K = tab["lam"].shape
    delta = np.where(tab["active"][0], tab["lam"][0], -np.inf)
    psi, margin = np.zeros((T, K), np.int64), np.full((T, K), np.inf)
    for t in range(1, T):
        for s in range(int(tab["n"][t])):
            vals = np.array([delta[p] - _cost(tab, t, p, s) for p in range(int(tab["n"][t - 1]))])
            order = np.argsort(-vals, kind="stable")
            psi[t, s] = order[0]
            margin[t, s] = vals[order[0]] - vals[order[1]] if vals.size > 1 else np.inf
        nd = np.full(K, -np.inf)
        for s in range(int(tab["n"][t])):
            nd[s] = delta[psi[t, s]] - _cost(tab, t, psi[t, s], s) + tab["lam"][t, s]
        delta = nd
    return psi, margin


def test_psi_is_the_running_sum_recursions():
    rng = np.random.default_rng(77)
    compared = 0
    for _ in range(40):
        T = 60
        cand, count, status, lp, params = _random_case(rng, T, kmax=4)
        tab = M.frame_table(cand, count, status, lp, None, params)
        D, prev, psi_m = None, None, []
        for t in range(T):
            cur = {n: tab[n][t:t + 1] for n in ("lf", "voiced", "active", "lam")}
            D, p = M.step(D, prev, cur, tab["k"])
            psi_m.append(p[0])
            prev = cur
        psi_m = np.array(psi_m)
        psi_r, margin = _running_sum_psi(tab)
        sel = tab["active"] & (margin > 1e-9)
        sel[0] = False
        assert np.array_equal(psi_m[sel], psi_r[sel])
        compared += int(sel.sum())
    assert compared > 5000


def test_a_dominant_leader_makes_the_state_forget():
    """Two different histories that agree on the leader: after one frame in which every state's best predecessor is the
    leader, D is bit for bit the same -- so a chunk entered from a wrong guess converges exactly, not approximately."""
    k = M.constants(M.DEFAULTS)
    prev = dict(lf=np.array([[np.log2(200.0), np.log2(400.0), np.log2(300.0), 0.0]]), voiced=np.array([[True, True, True, False]]),
                active=np.ones((1, 4), bool), lam=np.zeros((1, 4)))
    cur = dict(lf=np.array([[np.log2(210.0), np.log2(105.0), 0.0, 0.0]]), voiced=np.array([[True, True, False, False]]),
               active=np.array([[True, True, True, False]]), lam=np.array([[0.71, 0.62, 0.45, 0.0]]))
    D1 = np.array([[0.0, -5.0, -7.25, -3.5]])
    D2 = np.array([[0.0, -6.3, -2.1, -9.0]])
    a, pa = M.step(D1, prev, cur, k)
    b, pb = M.step(D2, prev, cur, k)
    assert np.all(pa[0, :3] == 0) and np.all(pb[0, :3] == 0)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    # ... and every later frame agrees too, while without the dominant leader the two histories stay apart
    c, _ = M.step(a, cur, cur, k)
    d, _ = M.step(b, cur, cur, k)
    assert np.array_equal(c.view(np.int64), d.view(np.int64))
    weak1, _ = M.step(np.array([[0.0, -5.0, -7.25, -0.05]]), prev, cur, k)     # the unvoiced state keeps its own history
    weak2, _ = M.step(np.array([[0.0, -5.0, -7.25, -0.06]]), prev, cur, k)
    assert not np.array_equal(weak1, weak2)


def test_model_outputs_follow_the_definition():
    cand = np.array([[[200.0, 0.9], [0.0, 0.2]], [[210.0, 0.8], [420.0, 0.85]], [[0.0, 0.0], [0.0, 0.0]]])
    count = np.array([2, 2, 0], np.int32)
    tab = M.frame_table(cand, count, None, None, None, dict(M.DEFAULTS, silence_threshold=0.0))
    assert list(tab["n"]) == [2, 3, 1]                         # frame 0 lists a 0 Hz entry: nothing appended
    path, index = M.pitch_path(cand, count, params=dict(M.DEFAULTS, silence_threshold=0.0))
    assert list(index) == [0, 0, -1]
    assert path[2, 0] == 0.0 and path[2, 1] == 0.45
