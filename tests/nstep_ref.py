"""numpy restatement of the n-step replay gather (csrc/nstep_terms.hpp, xa_ring_gather_nstep)
and of the two TD heads with a per-sample discount (xa_dqn_td_grad_n, xa_qr_td_grad_n).

The gather is written twice: `gather(..., dtype=np.float32)` in f32 in the header's stated
order (what the kernel must equal bit for bit) and `gather(..., dtype=np.float64)` (what the
f32 form is bounded against, and what seeds the f64 network oracle). gamma enters both as the
f32 the kernel is handed.

Rings are a dict of host arrays shaped like DeviceReplay's: states / new_states [n, cap, ...],
actions [n, cap, ...], rewards / dones [n, cap] f32; count [n] int64 appends per env. A slot is
env * cap + i.
"""
import numpy as np

import qr_ref as Q

EPS32 = 2.0 ** -24


def walk(count, cap, i, n_steps, dones_row):
    """(m_max, L) of slot i of an env with `count` appends and done row dones_row [cap]."""
    newest = (count - 1) % cap
    avail = ((newest - i) % cap) + 1
    m_max = min(n_steps, avail)
    L = m_max - 1
    for k in range(m_max):
        if dones_row[(i + k) % cap] != 0:
            L = k
            break
    return m_max, L


def fold(rewards, gamma, dtype):
    """R = r_L; R = r_k + gamma R for k = L - 1 .. 0, every operation rounded to dtype."""
    g = dtype(np.float32(gamma))
    R = dtype(rewards[-1])
    for r in rewards[-2::-1]:
        R = dtype(dtype(r) + dtype(g * R))
    return R


def discount(gamma, m, dtype):
    """g = gamma; g = g gamma another m - 1 times."""
    g0 = dtype(np.float32(gamma))
    g = g0
    for _ in range(m - 1):
        g = dtype(g * g0)
    return g


def gather(rings, count, slots, n_steps, gamma, dtype=np.float32):
    """Everything xa_ring_gather_nstep writes for `slots`, plus L [n_items]: dict(states,
    actions, rewards, dones, new_states, discounts, L)."""
    cap = rings['rewards'].shape[1]
    env, idx = np.divmod(np.asarray(slots, np.int64), cap)
    L = np.empty(len(env), np.int64)
    rew = np.empty(len(env), dtype)
    disc = np.empty(len(env), dtype)
    for b, (e, i) in enumerate(zip(env.tolist(), idx.tolist())):
        _, L[b] = walk(int(count[e]), cap, i, n_steps, rings['dones'][e])
        steps = [(i + k) % cap for k in range(L[b] + 1)]
        rew[b] = fold(rings['rewards'][e, steps], gamma, dtype)
        disc[b] = discount(gamma, int(L[b]) + 1, dtype)
    last = (idx + L) % cap
    return dict(states=rings['states'][env, idx], actions=rings['actions'][env, idx],
                rewards=rew, dones=rings['dones'][env, last],
                new_states=rings['new_states'][env, last], discounts=disc, L=L)


def fold_bound(rewards, gamma):
    """The f32-versus-f64 limit of fold() for an m-term chain: (2 m) eps sum_k gamma^k |r_k|
    (derivation: tests/test_nstep_ref.py)."""
    g = np.float64(np.float32(gamma))
    r = np.abs(np.asarray(rewards, np.float64))
    return 2 * len(r) * EPS32 * float((g ** np.arange(len(r)) * r).sum())


# ---- TD heads with a per-sample discount -----------------------------------------------------
def dqn_td(q, q_next_t, q_next_o, act, rew, done, discounts, huber, weights=None):
    """xa_dqn_td_grad_n in float64: dict(y, diff, dq [B, A], loss [B], td_abs [B]).
    y = v' discount_b + r, v' = 0 where done; MSE (huber <= 0): dq[b][a_b] = -2 diff / A,
    loss = diff^2 / A; Huber: dq = -clip(diff, +-delta) / A, loss = huber(diff) / A."""
    q, nt = np.asarray(q, np.float64), np.asarray(q_next_t, np.float64)
    B, A = q.shape
    rows = np.arange(B)
    if q_next_o is None:
        v = nt.max(1)
    else:
        v = nt[rows, np.asarray(q_next_o, np.float64).argmax(1)]
    v = np.where(np.asarray(done) != 0, 0.0, v)
    y = v * np.asarray(discounts, np.float64) + np.asarray(rew, np.float64)
    act = np.asarray(act, np.int64)
    diff = y - q[rows, act]
    if huber > 0:
        h = np.float64(np.float32(huber))
        L, Lp = Q.huber(diff, h)
    else:
        L, Lp = diff * diff, 2.0 * diff
    dq = np.zeros_like(q)
    dq[rows, act] = -Lp / A
    loss = L / A
    if weights is not None:
        w = np.asarray(weights, np.float64)
        dq, loss = dq * w[:, None], loss * w
    return dict(y=y, diff=diff, dq=dq, loss=loss, td_abs=np.abs(diff))


def qr_td(theta, theta_next_t, theta_next_o, act, rew, done, discounts, kappa, A, N,
          weights=None):
    """qr_ref.td with y_j = theta_next_t[b][a*][j] discount_b + r (qr_ref.targets takes one
    gamma for the batch); everything behind the targets is qr_ref's."""
    kappa = np.float64(np.float32(kappa))
    th, nt = Q._rows(theta, A, N), Q._rows(theta_next_t, A, N)
    B = th.shape[0]
    rows = np.arange(B)
    act = np.asarray(act, np.int64)
    a_star = Q.greedy(theta_next_t if theta_next_o is None else theta_next_o, A, N)
    v = np.where(np.asarray(done)[:, None] != 0, 0.0, nt[rows, a_star])
    y = v * np.asarray(discounts, np.float64)[:, None] + np.asarray(rew, np.float64)[:, None]
    th_a = th[rows, act]
    u, rho, g = Q.pairwise(th_a, y, kappa)
    loss = (rho.sum(2) / N).sum(1)
    d = np.zeros_like(th)
    d[rows, act] = -(g.sum(2) / N) / B
    td_abs = np.abs(y.sum(1) / N - th_a.sum(1) / N)
    if weights is not None:
        w = np.asarray(weights, np.float64)
        loss, d = loss * w, d * w[:, None, None]
    return dict(a_star=a_star, y=y, u=u, loss=loss, dtheta=d.reshape(B, A * N), td_abs=td_abs)


def step_discounts(B, gamma):
    """[B] f32: gamma^m with m cycling through 1, 2, 3, formed as the gather forms them."""
    return np.array([discount(gamma, 1 + b % 3, np.float32) for b in range(B)], np.float32)


def qr_case(B, A, N, kappa, seed=0):
    """qr_ref.case where it can serve the shape; (B, N) = (1, 1) holds a single pair, which
    cannot lie on both sides of kappa, so that shape gets qr_ref's generators without that one
    guarantee (the margins between compared mean-Q values are kept and asserted)."""
    if B * N >= 2:
        return Q.case(B, A, N, kappa, seed)
    rng = np.random.default_rng(100000 * B + 1000 * A + N + seed)
    c = dict(B=B, A=A, N=N, act=rng.integers(0, A, B).astype(np.int32))
    for key in ('theta', 'next_t', 'next_o'):
        c[key] = Q._net_rows(rng, B, A, N).reshape(B, A * N).astype(np.float32)
        assert Q.margin(c[key], A, N) >= Q.MARGIN, key
    c['rew'] = rng.normal(size=B).astype(np.float32)
    c['done'] = np.zeros(B, np.float32)
    c['weights'] = rng.uniform(0.05, 1.0, B).astype(np.float32)
    return c


def dqn_case(B, A, seed=0):
    """Fixed [B, A] inputs of the scalar head: every row's Q values of the next state are at
    least 0.05 apart (online and target), so an argmax is the same in f32 and f64; row 0 is
    done."""
    rng = np.random.default_rng(1000 * B + A + seed)

    def rows():
        level = np.stack([rng.permutation(A) for _ in range(B)]) * 0.1
        return (level + rng.uniform(0.0, 0.05, (B, A)) - 0.2).astype(np.float32)

    c = dict(B=B, A=A, q=rng.normal(size=(B, A)).astype(np.float32), next_t=rows(),
             next_o=rows(), act=rng.integers(0, A, B).astype(np.int32),
             rew=rng.normal(size=B).astype(np.float32),
             done=(rng.random(B) < 0.3).astype(np.float32),
             weights=rng.uniform(0.05, 1.0, B).astype(np.float32))
    c['done'][0] = 1.0
    if B > 1:
        c['done'][-1] = 0.0
    for key in ('next_t', 'next_o'):
        assert np.diff(np.sort(c[key].astype(np.float64), axis=1), axis=1).min() >= 0.04
    return c
