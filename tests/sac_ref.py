"""Float64 numpy restatement of Soft Actor-Critic's arithmetic (xagents_amd/csrc/sac_terms.hpp):
the tanh-squashed Gaussian sample and log-density, the soft critic target, the critic / actor /
temperature losses and their analytic gradients, and one whole gradient step through the
float64 layers of oracle/nets_f64.py. Test infrastructure only."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / 'oracle'))

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def f64(x):
    return np.asarray(x, np.float64)


def clamp_log_std(log_std):
    return np.clip(f64(log_std), LOG_STD_MIN, LOG_STD_MAX)


def clamp_grad(log_std):
    """0 strictly outside [LOG_STD_MIN, LOG_STD_MAX], 1 inside and at the bounds."""
    log_std = f64(log_std)
    return 1.0 - ((log_std < LOG_STD_MIN) | (log_std > LOG_STD_MAX))


def softplus(x):
    x = f64(x)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def log_one_minus_tanh2(u):
    """log(1 - tanh(u)^2) in the overflow-free form 2 (log 2 - u - softplus(-2 u))."""
    u = f64(u)
    return 2.0 * (np.log(2.0) - u - softplus(-2.0 * u))


def log_one_minus_tanh2_naive(u):
    return np.log(1.0 - np.tanh(f64(u)) ** 2)


def sample(mean, log_std, eps):
    """(actions [n, A], logp [n], u) of the squashed Gaussian at the given eps."""
    mean, eps = f64(mean), f64(eps)
    ls = clamp_log_std(log_std)
    u = mean + np.exp(ls) * eps
    terms = -0.5 * eps * eps - ls - HALF_LOG_2PI - log_one_minus_tanh2(u)
    return np.tanh(u), terms.sum(1), u


def soft_target(r, done, gamma, tv1, tv2, log_alpha, logp_next):
    soft = np.minimum(f64(tv1), f64(tv2)) - np.exp(log_alpha) * f64(logp_next)
    return f64(r) + (1.0 - f64(done)) * gamma * soft


def td_term(e, delta):
    """(loss term, derivative) of the TD error e: MSE, or Huber(delta) when delta > 0."""
    e = f64(e)
    if delta and delta > 0:
        ae = np.abs(e)
        return (np.where(ae <= delta, 0.5 * e * e, delta * (ae - 0.5 * delta)),
                np.clip(e, -delta, delta))
    return e * e, 2.0 * e


def td_grad(v1, v2, tv1, tv2, logp_next, log_alpha, r, done, gamma, delta=0.0):
    """(dv1, dv2, per-row loss): the critics' losses are batch sums."""
    y = soft_target(r, done, gamma, tv1, tv2, log_alpha, logp_next)
    l1, d1 = td_term(f64(v1) - y, delta)
    l2, d2 = td_term(f64(v2) - y, delta)
    return d1, d2, l1 + l2


def actor_rows(q1, q2, logp, log_alpha):
    """Per-row actor loss alpha logp - min(q1, q2); the batch loss is its mean."""
    return np.exp(log_alpha) * f64(logp) - np.minimum(f64(q1), f64(q2))


def actor_seed(q1, q2):
    """d(-mean Qmin)/dq1, /dq2: -1 / B on the critic holding the minimum (ties: critic 1)."""
    q1, q2 = f64(q1), f64(q2)
    first = (q1 <= q2).astype(np.float64)
    return -first / q1.shape[0], -(1.0 - first) / q1.shape[0]


def head_grad(dqa, actions, eps, log_std, log_alpha):
    """(dmean, dlog_std) [B, A] from dqa = d(-mean Qmin)/d action."""
    dqa, a, eps = f64(dqa), f64(actions), f64(eps)
    ab = np.exp(log_alpha) / a.shape[0]
    du = dqa * (1.0 - a * a) + ab * 2.0 * a
    return du, clamp_grad(log_std) * (du * np.exp(clamp_log_std(log_std)) * eps - ab)


def temperature_loss(log_alpha, logp, target_entropy):
    return -np.mean(log_alpha * (f64(logp) + target_entropy))


def temperature_grad(logp, target_entropy):
    return -np.mean(f64(logp) + target_entropy)


# ---- one gradient step through the float64 layers -------------------------------------
def _fw(m, theta, x):
    import nets_f64 as O
    return O.forward(m.layers, theta, x, m.input_shape)


def gradient_step(agent, th, tt, log_alpha, batch, eps, eps_next, lr, alpha_lr, tau, gamma,
                  auto, critics_for_actor=None):
    """The f64 replay of SAC.update_weights(1) from first-step Adam state (zero moments).
    th = [actor, critic1, critic2] parameters, tt = [target critic 1, 2], batch =
    (s, a, r, d, s2), eps / eps_next the draws for a_pi / a'. critics_for_actor: critic
    parameters the actor step differentiates through (default: this function's own updated
    critics). Returns a dict of the raw gradients, the new parameters and the targets."""
    import nets_f64 as O
    import oracle as OR
    adam = lambda p, g, rate: OR.keras_adam_f64(p, 0, 0, g, 1, rate, 0.9, 0.999, 1e-7)[0]  # noqa: E731
    s, a, r, d, s2 = (f64(x) for x in batch)
    B = s.shape[0]
    act, crit = agent.actor, agent.critic
    heads = lambda o: (o[act.outputs[0]], o[act.outputs[1]])  # noqa: E731
    out = {}
    # critics
    _, o2 = _fw(act, th[0], s2)
    a2, logp2, _ = sample(*heads(o2), eps_next)
    s2a2 = np.concatenate([s2, a2], 1)
    tv = [_fw(crit, t, s2a2)[1][crit.outputs[0]][:, 0] for t in tt]
    sa = np.concatenate([s, a], 1)
    fwd = [_fw(crit, th[i], sa) for i in (1, 2)]
    v = [o[crit.outputs[0]][:, 0] for _, o in fwd]
    dv1, dv2, _ = td_grad(v[0], v[1], tv[0], tv[1], logp2, log_alpha, r, d, gamma,
                          agent.huber_delta or 0.0)
    new = [None, None, None]
    for i, dv in ((1, dv1), (2, dv2)):
        x64, o = fwd[i - 1]
        g = O.backward(crit.layers, th[i], x64, o, {crit.outputs[0]: dv[:, None]})
        out[f'g_critic{i}'] = g
        new[i] = adam(th[i], g, lr)
    out['logp_next'] = logp2
    # actor through the updated critics
    cs = critics_for_actor if critics_for_actor is not None else new[1:]
    xa, oa = _fw(act, th[0], s)
    mean, log_std = heads(oa)
    api, logp, _ = sample(mean, log_std, eps)
    spa = np.concatenate([s, api], 1)
    fq = [_fw(crit, c, spa) for c in cs]
    q = [o[crit.outputs[0]][:, 0] for _, o in fq]
    dq = actor_seed(q[0], q[1])
    dqa = np.zeros_like(api)
    for c, (xc, oc), dqi in zip(cs, fq, dq):
        _, dx = O.backward(crit.layers, c, xc, oc, {crit.outputs[0]: dqi[:, None]},
                           want_input_grad=True)
        dqa += dx[:, s.shape[1]:]
    dmean, dlog_std = head_grad(dqa, api, eps, log_std, log_alpha)
    ga = O.backward(act.layers, th[0], xa, oa, {act.outputs[0]: dmean, act.outputs[1]: dlog_std})
    out['g_actor'] = ga
    out['logp'] = logp
    out['q'] = q
    new[0] = adam(th[0], ga, lr)
    g_alpha = temperature_grad(logp, agent.target_entropy)
    out['g_log_alpha'] = g_alpha
    out['log_alpha'] = adam(np.array([log_alpha]), np.array([g_alpha]), alpha_lr)[0] \
        if auto else log_alpha
    out['theta'] = new
    out['targets'] = [(1.0 - tau) * t + tau * n for t, n in zip(tt, new[1:])]
    assert B == a.shape[0]
    return out
