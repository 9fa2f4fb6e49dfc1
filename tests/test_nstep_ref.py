"""tests/nstep_ref.py pinned on the CPU: against a brute-force replay of what was appended, and
its f32 form against its f64 form by a derived limit.

The brute force keeps, per env, the Python list of every transition ever appended and a
deque(maxlen = capacity) of the append numbers still stored (ReplayBuffer1's deque). Append
number t lives in ring slot t mod capacity. The n-step transition of a stored append t0 walks
the list: t0, t0 + 1, ... while the append exists (t < count), for at most n_steps, stopping
behind the first done.

The limit of the f32 Horner chain R = r_0 + g (r_1 + g (... + g r_L)) against f64, m = L + 1
terms, eps = 2^-24, g the same f32 gamma in both: r_k reaches R through k multiplies by g and
k adds, each one rounding (1 + d), |d| <= eps, so its coefficient is g^k (1 + d)^(2 k) and
    |R32 - R| <= sum_k ((1 + eps)^(2 k) - 1) g^k |r_k| <= (2 m) eps sum_k g^k |r_k|
for k <= m - 1 <= 63: (1 + eps)^(2 k) - 1 <= 2 k eps (1 + 2 k eps) < 2 m eps. The f64 form's own
rounding (2^-53 per operation) is eight orders below. m = 1 gives R = r_0 exactly. The
discount g^m takes m - 1 roundings: |g32 - g^m| <= m eps g^m.
"""
from collections import deque

import numpy as np
import pytest

import nstep_ref as NS
import qr_ref as Q

GAMMA = 0.99


def _appended(rng, n_envs, cap, counts, p_done):
    """Per env the list of appended transitions (state id, action, reward, done, next state
    id), and the rings they leave behind."""
    rings = dict(states=np.zeros((n_envs, cap), np.int32), new_states=np.zeros((n_envs, cap), np.int32),
                 actions=np.zeros((n_envs, cap), np.int32),
                 rewards=np.zeros((n_envs, cap), np.float32),
                 dones=np.zeros((n_envs, cap), np.float32))
    logs, stored = [], []
    for e in range(n_envs):
        log, dq = [], deque(maxlen=cap)
        for t in range(counts[e]):
            tr = (1000 * e + t, int(rng.integers(0, 4)), np.float32(rng.normal()),
                  np.float32(rng.random() < p_done), 1000 * e + t + 500)
            log.append(tr)
            dq.append(t)
            s = t % cap
            rings['states'][e, s], rings['actions'][e, s] = tr[0], tr[1]
            rings['rewards'][e, s], rings['dones'][e, s] = tr[2], tr[3]
            rings['new_states'][e, s] = tr[4]
        logs.append(log)
        stored.append(dq)
    return logs, stored, rings


def _brute(log, t0, n_steps):
    """(first, rewards walked, last) from the list of appended transitions."""
    walked = []
    for t in range(t0, min(t0 + n_steps, len(log))):
        walked.append(log[t])
        if log[t][3] != 0:
            break
    return walked


@pytest.mark.parametrize('n_steps', [1, 2, 3, 5, 7])
@pytest.mark.parametrize('p_done', [0.0, 0.3, 1.0])
def test_restatement_is_the_walk_over_what_was_appended(n_steps, p_done):
    cap, counts = 7, (1, 5, 7, 12, 30)
    rng = np.random.default_rng(10 * n_steps + int(10 * p_done))
    logs, stored, rings = _appended(rng, len(counts), cap, counts, p_done)
    count = np.asarray(counts, np.int64)
    slots, origin = [], []
    for e, dq in enumerate(stored):
        for t0 in dq:  # every stored transition, oldest first
            slots.append(e * cap + t0 % cap)
            origin.append((e, t0))
    assert len(slots) == sum(min(c, cap) for c in counts)
    g32 = NS.gather(rings, count, slots, n_steps, GAMMA, np.float32)
    g64 = NS.gather(rings, count, slots, n_steps, GAMMA, np.float64)
    assert g32['rewards'].dtype == np.float32 and g32['discounts'].dtype == np.float32
    g = np.float64(np.float32(GAMMA))
    seen_m = set()
    for b, (e, t0) in enumerate(origin):
        walked = _brute(logs[e], t0, n_steps)
        m = len(walked)
        seen_m.add(m)
        assert g32['L'][b] == g64['L'][b] == m - 1
        for got in (g32, g64):
            assert got['states'][b] == walked[0][0] and got['actions'][b] == walked[0][1]
            assert got['new_states'][b] == walked[-1][4] and got['dones'][b] == walked[-1][3]
        r = np.array([w[2] for w in walked], np.float64)
        want = float((g ** np.arange(m) * r).sum())
        scale = float((g ** np.arange(m) * np.abs(r)).sum())
        assert abs(g64['rewards'][b] - want) <= 1e-13 * max(scale, 1e-300)
        assert abs(g64['discounts'][b] - g ** m) <= 1e-13
        # f32 against f64 by the derived limits
        lim = NS.fold_bound(r, GAMMA)
        assert lim == pytest.approx(2 * m * NS.EPS32 * scale)
        assert abs(np.float64(g32['rewards'][b]) - g64['rewards'][b]) <= lim
        assert abs(np.float64(g32['discounts'][b]) - g64['discounts'][b]) <= m * NS.EPS32 * g ** m
        if m == 1:
            assert g32['rewards'][b].tobytes() == walked[0][2].tobytes()
            assert g32['discounts'][b].tobytes() == np.float32(GAMMA).tobytes()
    if p_done == 0.0:  # the walk is cut by the ring's head only
        assert seen_m == set(range(1, n_steps + 1))
    if p_done == 1.0:
        assert seen_m == {1}


def test_walk_never_passes_the_newest_entry_of_a_wrapped_ring():
    """count 12 at capacity 7: newest = slot 4, oldest = slot 5. From slot 3 two steps are
    left, from slot 4 one, from slot 5 (the oldest) seven."""
    none = np.zeros(7, np.float32)
    assert NS.walk(12, 7, 3, 5, none) == (2, 1)
    assert NS.walk(12, 7, 4, 5, none) == (1, 0)
    assert NS.walk(12, 7, 5, 7, none) == (7, 6)
    assert NS.walk(12, 7, 5, 3, none) == (3, 2)
    done = none.copy()
    done[[6, 1]] = 1.0  # two dones inside the walk from slot 5: it stops at the first
    assert NS.walk(12, 7, 5, 7, done) == (7, 1)
    assert NS.walk(12, 7, 0, 7, done) == (5, 1)
    # not yet wrapped: count 5, newest = slot 4
    assert NS.walk(5, 7, 0, 7, none) == (5, 4)
    assert NS.walk(1, 7, 0, 3, none) == (1, 0)


def test_long_chain_stays_inside_its_limit():
    """n_steps = 64, rewards of mixed sign and scale."""
    rng = np.random.default_rng(64)
    for _ in range(50):
        r = (rng.normal(size=64) * 10.0 ** rng.integers(-3, 4, 64)).astype(np.float32)
        err = abs(np.float64(NS.fold(r, GAMMA, np.float32)) - NS.fold(r, GAMMA, np.float64))
        assert err <= NS.fold_bound(r, GAMMA)
    assert abs(np.float64(NS.discount(GAMMA, 64, np.float32)) -
               NS.discount(GAMMA, 64, np.float64)) <= 64 * NS.EPS32 * 0.99 ** 64


@pytest.mark.parametrize('B,A,N', [(1, 2, 1), (5, 6, 64), (65, 2, 65)])
def test_per_row_heads_reduce_to_the_one_gamma_forms(B, A, N):
    """With every discount equal to gamma the per-row quantile head is qr_ref.td, and the
    scalar head is the reference's y = v' gamma + r."""
    c = NS.qr_case(B, A, N, 1.0)
    disc = np.full(B, np.float32(GAMMA), np.float32)
    for online in (None, c['next_o']):
        a = NS.qr_td(c['theta'], c['next_t'], online, c['act'], c['rew'], c['done'], disc, 1.0,
                     A, N, c['weights'])
        b = Q.td(c['theta'], c['next_t'], online, c['act'], c['rew'], c['done'], GAMMA, 1.0, A,
                 N, c['weights'])
        for key in ('a_star', 'y', 'loss', 'dtheta', 'td_abs'):
            np.testing.assert_array_equal(a[key], b[key])
    d = NS.dqn_case(B, A)
    r = NS.dqn_td(d['q'], d['next_t'], None, d['act'], d['rew'], d['done'], disc, 0.0)
    v = np.where(d['done'] != 0, 0.0, d['next_t'].astype(np.float64).max(1))
    y = v * np.float64(np.float32(GAMMA)) + d['rew']
    np.testing.assert_array_equal(r['y'], y)
    rows = np.arange(B)
    np.testing.assert_array_equal(r['dq'][rows, d['act']], -2.0 * (y - d['q'][rows, d['act']]) / A)
    assert np.count_nonzero(r['dq']) <= B
    # Huber: clipped derivative, the same target
    h = NS.dqn_td(d['q'], d['next_t'], d['next_o'], d['act'], d['rew'], d['done'], disc, 0.5)
    assert np.abs(h['dq']).max() <= 0.5 / A + 1e-15
