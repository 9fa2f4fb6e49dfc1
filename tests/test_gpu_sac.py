"""GPU tests of Soft Actor-Critic (xagents_amd/sac, csrc/sac.hip): the four kernels against
the float64 restatement (tests/sac_ref.py), one gradient step against its f64 replay from the
batch and the draws the device made, captured phases against eager launches, the training
loop, play and checkpoints.

Kernel tolerances, from the f32 formats (ulp = 2^-23 relative, one rounding = half of it):
* actions: xa_tanhf is within 5 ulp of tanh (xa_common.hpp) and its results lie in [-1, 1],
  so 5 * 2^-24 = 3.0e-7; u = mean + exp(ls) eps carries <= 4 ulp(u) (two roundings, xa_expf
  within 2 ulp), which tanh scales by 1 - tanh(u)^2: 4 * 2^-23 * max_u |u| (1 - tanh(u)^2) =
  4 * 1.19e-7 * 0.448 = 2.1e-7. Sum 5.1e-7 -> ACT_ATOL = 6e-7.
* logp: the bound tests/test_gpu_distributions.py applies to xa_diag_gaussian's log-prob,
  rtol = atol = 1e-5.
* every other output is a short sum of products; an f32 evaluation of it carries a few ulps
  of the sum of the |terms| (not of the possibly cancelling result), the way
  tests/test_gpu_configs.py bounds dq: err <= ULPS * 2^-23 * sum |terms| with ULPS = 8 (at
  most 8 roundings and the 2 ulp of xa_expf in alpha / exp(ls) on any path), error carried
  in from an earlier sum propagated through the factor that multiplies it.
"""
import random
from pathlib import Path

import numpy as np
import pytest
import torch

import sac_ref as R

pytestmark = pytest.mark.gpu

ACT_ATOL = 6e-7
LOGP_TOL = dict(rtol=1e-5, atol=1e-5)
ULP = 8 * 2.0 ** -23
# 1, not a multiple of the 64-row workgroups (nor of actor_seed's 256 threads), and more
# than one workgroup of either
ROWS = (1, 37, 300)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _dev(device, x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(device)


def _rel(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


def _step_close(got, th0, ref, lr=1e-3, tol=2e-2):
    err = np.abs((got - th0) - (ref - th0)).max() / lr
    assert err < tol, f'update mismatch {err:.3g} (units of lr)'


def _call(name, *args):
    from xagents_amd._lib import call, stream
    call(name, *args, stream())
    torch.cuda.synchronize()


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- 1. kernels ------------------------------------------------------------------------
def _head_inputs(n, A, seed):
    """mean / log_std with rows whose |u| is near 10 and log_std at, inside and beyond both
    clamp bounds."""
    rng = np.random.default_rng(seed)
    mean = rng.normal(size=(n, A)).astype(np.float32)
    log_std = np.resize(np.array([-25.0, -20.0, -3.0, 0.0, 2.0, 2.5, -1.0], np.float32),
                        (n, A)).copy()
    far = np.arange(n) % 5 == 0
    mean[far] = np.where(rng.random((int(far.sum()), A)) < 0.5, -10.0, 10.0) + \
        0.1 * mean[far]
    log_std[far] = np.minimum(log_std[far], -1.0)
    return mean, log_std


def _sample(device, mean, log_std, ctr=None, seed=99, eps_in=None, deterministic=0, ld=None):
    n, A = mean.shape
    ld = ld or A
    out = torch.full((n, ld), 7.0, device=device)
    eps_out = torch.full((n, A), 7.0, device=device)
    logp = torch.full((n,), 7.0, device=device)
    tm, tl = _dev(device, mean), _dev(device, log_std)
    te = None if eps_in is None else _dev(device, eps_in)
    _call('xa_sac_sample', tm.data_ptr(), A, tl.data_ptr(), A, n, A, _ptr(te), _ptr(ctr), seed,
          deterministic, out.data_ptr(), ld, eps_out.data_ptr(), logp.data_ptr())
    return out.cpu().numpy(), eps_out.cpu().numpy(), logp.cpu().numpy()


@pytest.mark.parametrize('A', [1, 4])
@pytest.mark.parametrize('n', ROWS)
def test_sample_vs_f64(device, n, A):
    """Actions and logp from the eps the launch drew, into an output wider than A (the action
    columns of an [s, a] buffer); the deterministic head; a supplied eps_in reproduces the
    drawn run bit for bit."""
    mean, log_std = _head_inputs(n, A, 10 * n + A)
    ctr = torch.full((1,), 5, dtype=torch.int64, device=device)
    ld = A + 3
    act, eps, logp = _sample(device, mean, log_std, ctr, ld=ld)
    assert (act[:, A:] == 7.0).all()  # nothing written past the action columns
    assert np.isfinite(eps).all() and (n * A < 8 or eps.std() > 0.3)
    a64, lp64, u = R.sample(mean, log_std, eps)
    if n >= 5:
        assert np.abs(u).max() > 9.0
    np.testing.assert_allclose(act[:, :A], a64, rtol=0, atol=ACT_ATOL)
    assert np.isfinite(logp).all()
    np.testing.assert_allclose(logp, lp64, **LOGP_TOL)
    # eps_in: the same bits, and no draw (a null counter is accepted)
    act2, eps2, logp2 = _sample(device, mean, log_std, None, eps_in=eps, ld=ld)
    for x, y in ((act, act2), (eps, eps2), (logp, logp2)):
        assert x.tobytes() == y.tobytes()
    # deterministic: a = tanh(mean), eps = 0, the density of the mode
    act3, eps3, logp3 = _sample(device, mean, log_std, None, deterministic=1, ld=ld)
    assert not eps3.any()
    a64, lp64, _ = R.sample(mean, log_std, np.zeros_like(mean))
    np.testing.assert_allclose(act3[:, :A], np.tanh(mean.astype(np.float64)), rtol=0,
                               atol=ACT_ATOL)
    np.testing.assert_allclose(logp3, lp64, **LOGP_TOL)


def test_sample_draw_statistics(device):
    """4096 x 4 draws: mean and standard deviation within 5 standard errors (1 / sqrt(N) and
    1 / sqrt(2 N)) of 0 and 1; the same (seed, counter) reproduces the bits, a bumped
    counter does not."""
    n, A = 4096, 4
    zero = np.zeros((n, A), np.float32)
    ctr = torch.full((1,), 11, dtype=torch.int64, device=device)
    _, eps, _ = _sample(device, zero, zero, ctr)
    N = n * A
    assert abs(eps.mean()) < 5 / np.sqrt(N)
    assert abs(eps.std() - 1.0) < 5 / np.sqrt(2 * N)
    _, again, _ = _sample(device, zero, zero, ctr)
    assert again.tobytes() == eps.tobytes()
    from xagents_amd import kernels
    kernels.counter_bump(ctr)
    _, other, _ = _sample(device, zero, zero, ctr)
    assert int(ctr.item()) == 12 and (other != eps).mean() > 0.99


@pytest.mark.parametrize('huber', [0.0, 0.5])
@pytest.mark.parametrize('B', ROWS)
def test_td_grad_vs_f64(device, B, huber):
    rng = np.random.default_rng(B)
    v1, v2, tv1, tv2, r = (rng.normal(size=B).astype(np.float32) for _ in range(5))
    logp2 = (3 * rng.normal(size=B)).astype(np.float32)
    done = (rng.random(B) < 0.3).astype(np.float32)
    la = np.float32(-0.7)
    t = {k: _dev(device, x) for k, x in dict(v1=v1, v2=v2, tv1=tv1, tv2=tv2, r=r, lp=logp2,
                                             d=done, la=[la]).items()}
    out = {k: torch.full((B + 1,), 7.0, device=device) for k in ('dv1', 'dv2', 'loss')}
    _call('xa_sac_td_grad', t['v1'].data_ptr(), t['v2'].data_ptr(), t['tv1'].data_ptr(),
          t['tv2'].data_ptr(), t['lp'].data_ptr(), t['la'].data_ptr(), t['r'].data_ptr(),
          t['d'].data_ptr(), B, 0.99, huber, out['dv1'].data_ptr(), out['dv2'].data_ptr(),
          out['loss'].data_ptr())
    d1, d2, loss = R.td_grad(v1, v2, tv1, tv2, logp2, la, r, done, np.float32(0.99), huber)
    # |terms| of e = v - r - (1 - d) gamma (min tv - alpha logp')
    alpha = np.exp(np.float64(la))
    tail = np.abs(r) + (1 - done) * 0.99 * (np.abs(np.minimum(tv1, tv2)) + alpha * np.abs(logp2))
    for got, want, v in ((out['dv1'], d1, v1), (out['dv2'], d2, v2)):
        g = _np(got)
        assert g[B] == 7.0
        de = ULP * (np.abs(v) + tail)
        assert (np.abs(g[:B] - want) <= 2 * de + ULP * np.abs(want)).all()
    y = R.soft_target(r, done, 0.99, tv1, tv2, la, logp2)
    # a term's slope in e is at most 2 max(|e|, delta): an error de in e moves it by
    # 2 (|e| + delta) de + de^2
    dl = 0.0
    for v in (v1, v2):
        e, de = np.abs(v - y), ULP * (np.abs(v) + tail)
        dl = dl + 2 * (e + huber) * de + de * de
    assert (np.abs(_np(out['loss'])[:B] - loss) <= dl + ULP * np.abs(loss)).all()


@pytest.mark.parametrize('B', ROWS)
def test_actor_seed_vs_f64(device, B):
    """Seeds (exact, with a q1 == q2 tie row going to critic 1), the per-row actor loss and
    the temperature gradient's one-workgroup reduction at every row count."""
    rng = np.random.default_rng(100 + B)
    q1, q2 = rng.normal(size=B).astype(np.float32), rng.normal(size=B).astype(np.float32)
    q2[B // 2] = q1[B // 2]
    logp = (3 * rng.normal(size=B) - 1).astype(np.float32)
    la, te = np.float32(0.3), np.float32(-4.0)
    t = [_dev(device, x) for x in (q1, q2, logp, [la])]
    dq1, dq2, loss = (torch.full((B + 1,), 7.0, device=device) for _ in range(3))
    dla = torch.full((2,), 7.0, device=device)
    _call('xa_sac_actor_seed', *(x.data_ptr() for x in t), B, float(te), dq1.data_ptr(),
          dq2.data_ptr(), loss.data_ptr(), dla.data_ptr())
    w1, w2 = R.actor_seed(q1, q2)
    seed = np.float32(-1.0) / np.float32(B)
    g1, g2 = dq1.cpu().numpy(), dq2.cpu().numpy()
    assert g1[B] == 7.0 and g2[B] == 7.0 and _np(dla)[1] == 7.0
    np.testing.assert_array_equal(g1[:B], np.where(w1 != 0, seed, np.float32(0)))
    np.testing.assert_array_equal(g2[:B], np.where(w2 != 0, seed, np.float32(0)))
    assert g1[B // 2] == seed and g2[B // 2] == 0.0
    rows = R.actor_rows(q1, q2, logp, la)
    terms = np.exp(np.float64(la)) * np.abs(logp) + np.abs(np.minimum(q1, q2))
    assert (np.abs(_np(loss)[:B] - rows) <= ULP * terms).all()
    # each row's logp + target_entropy is one f32 rounding (half an ulp of at most
    # |logp| + |target_entropy|), the sum runs in f64, the result is rounded to f32 once
    want = R.temperature_grad(logp, te)
    bound = 2.0 ** -24 * (np.mean(np.abs(logp) + abs(te)) + abs(want)) + 1e-12
    assert abs(_np(dla)[0] - want) <= bound, (_np(dla)[0], want, bound)


@pytest.mark.parametrize('A', [1, 4])
@pytest.mark.parametrize('B', ROWS)
def test_head_grad_vs_f64(device, B, A):
    rng = np.random.default_rng(7 * B + A)
    mean, log_std = _head_inputs(B, A, B + A)
    eps = rng.normal(size=(B, A)).astype(np.float32)
    act = np.tanh(mean + np.exp(R.clamp_log_std(log_std)) * eps).astype(np.float32)
    ld = A + 2
    da = np.zeros((B, ld), np.float32)
    da[:, :A] = rng.normal(size=(B, A)) / B
    actions = np.zeros((B, ld), np.float32)
    actions[:, :A] = act
    la = np.float32(-1.2)
    t = [_dev(device, x) for x in (da, actions, eps, log_std, [la])]
    dmean, dls = torch.full((B * A + 1,), 7.0, device=device), \
        torch.full((B * A + 1,), 7.0, device=device)
    _call('xa_sac_head_grad', t[0].data_ptr(), ld, t[1].data_ptr(), ld, t[2].data_ptr(),
          t[3].data_ptr(), A, t[4].data_ptr(), B, A, dmean.data_ptr(), dls.data_ptr())
    wm, wl = R.head_grad(da[:, :A], act, eps, log_std, la)
    gm, gl = _np(dmean), _np(dls)
    assert gm[B * A] == 7.0 and gl[B * A] == 7.0
    gm, gl = gm[:B * A].reshape(B, A), gl[:B * A].reshape(B, A)
    ab = np.exp(np.float64(la)) / B
    a64 = act.astype(np.float64)
    s_du = np.abs(da[:, :A]) * (1 + a64 * a64) + ab * 2 * np.abs(a64)
    assert (np.abs(gm - wm) <= ULP * s_du).all()
    k = np.exp(R.clamp_log_std(log_std)) * np.abs(eps)
    assert (np.abs(gl - wl) <= ULP * (s_du * k + np.abs(wm) * k + ab)).all()
    outside = (log_std < R.LOG_STD_MIN) | (log_std > R.LOG_STD_MAX)
    assert outside.any() and not gl[outside].any() and (gl[~outside] != 0).all()


# ---- 2. the agent ----------------------------------------------------------------------
ENVS = {'Pendulum-v1': {}, 'BipedalWalker-v3': dict(t_rec=64)}


def _agent(device, env_id='BipedalWalker-v3', n=4, gradient_steps=1, tau=0.05, alpha='auto',
           env_kwargs=None, split_critics=True, **kwargs):
    from xagents_amd import SAC
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    envs = create_envs(env_id, n, device=device, seed=4, **(env_kwargs or ENVS[env_id]))
    kw = dict(seed=7, device=device, optimizer_kwargs=dict(learning_rate=1e-3))
    actor = create_model(envs, 'sac', 'actor_model', **kw)
    critic = create_model(envs, 'sac', 'critic_model', **kw)
    bufs = create_buffers('sac', 8 * n, 2 * n, n, initial_size=4 * n)
    agent = SAC(envs, actor, critic, bufs, gradient_steps=gradient_steps, tau=tau, alpha=alpha,
                seed=3, quiet=True, gamma=0.99, **kwargs)
    if split_critics:
        # a seeded model draws critic 2 equal to critic 1 (every min would tie): move it
        g = torch.Generator().manual_seed(1)
        scale = 1.0 + 0.2 * torch.randn(agent.critic2.n_params, generator=g)
        agent.critic2.theta.mul_(scale.to(device))
        agent.target_critic2.theta.copy_(agent.critic2.theta)
    return agent


def _models(agent):
    return [agent.actor, agent.critic1, agent.critic2]


@pytest.mark.parametrize('env_id,n,alpha', [
    ('Pendulum-v1', 4, 'auto'), ('Pendulum-v1', 50, 'auto'), ('BipedalWalker-v3', 4, 'auto'),
    ('BipedalWalker-v3', 50, 'auto'), ('Pendulum-v1', 4, 0.2), ('BipedalWalker-v3', 4, 0.2)])
def test_one_gradient_step_vs_f64(device, env_id, n, alpha):
    """n = 4: batch 8 (one ragged row tile); n = 50: batch 100. A = 1 (Pendulum) and A = 4.
    The raw gradients g_critic / g_critic2 / g_actor at 1e-4 relative (a first Adam step from
    zero moments is ~ lr sign(g), so the step check alone would pass a gradient off by a
    factor; the actor's through the device's own updated critics, where an element whose
    critic gradient is ~0 took an Adam step that f32 and f64 may round apart), then the
    applied steps of the actor, both critics and log_alpha within 2e-2 of the learning rate,
    and the Polyak targets from the updated parameters. alpha = 0.2: log_alpha keeps its
    bits."""
    agent = _agent(device, env_id, n=n, alpha=alpha)
    auto = alpha == 'auto'
    tau = 0.05
    assert agent.batch_size == 2 * n and agent.A == (1 if env_id == 'Pendulum-v1' else 4)
    assert agent._fused_args() is None and agent._fused_act_args() is None
    assert agent.model_groups == [(agent.critic1, agent.target_critic1),
                                  (agent.critic2, agent.target_critic2)]
    assert not hasattr(agent, 'target_actor')
    assert agent.target_entropy == -agent.A
    agent.fill_buffers()
    th0 = [_np(m.theta) for m in _models(agent)]
    tt0 = [_np(agent.target_critic1.theta), _np(agent.target_critic2.theta)]
    la0 = agent.log_alpha.clone()
    assert float(la0.item()) == float(np.float32(np.log(1.0 if auto else 0.2)))
    c0 = int(agent.rng_counter.item())
    agent.update_weights(1)
    torch.cuda.synchronize()
    assert int(agent.rng_counter.item()) == c0 + 2  # one bump per draw: a', a_pi
    batch = [_np(x) for x in (agent.s, agent.a, agent.r, agent.d, agent.s2)]
    eps, eps_next = _np(agent.eps), _np(agent.eps_next)
    assert eps.std() > 0.1 or eps.size < 16
    assert not np.array_equal(eps, eps_next)
    args = (agent, th0, tt0, float(la0.item()), batch, eps, eps_next, 1e-3, 1e-3, tau, 0.99, auto)
    ref = R.gradient_step(*args)
    np.testing.assert_allclose(_np(agent.logp_next), ref['logp_next'], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(_np(agent.logp), ref['logp'], rtol=1e-4, atol=1e-4)
    for name, g in (('g_critic1', agent.g_critic), ('g_critic2', agent.g_critic2)):
        e = _rel(_np(g), ref[name])
        assert e < 1e-4, f'{name}: raw gradient {e:.2e}'
    dev_critics = [_np(agent.critic1.theta), _np(agent.critic2.theta)]
    own = R.gradient_step(*args, critics_for_actor=dev_critics)
    # both seeds are exercised: neither critic holds every minimum
    first = own['q'][0] <= own['q'][1]
    assert n < 50 or (first.any() and not first.all())
    e = _rel(_np(agent.g_actor), own['g_actor'])
    assert e < 1e-4, f'actor: raw gradient {e:.2e}'
    for m, t0, want in zip(_models(agent), th0, ref['theta']):
        _step_close(_np(m.theta), t0, want)
    if auto:
        g = float(agent.g_log_alpha.item())
        assert abs(g - own['g_log_alpha']) <= 1e-4 * max(1.0, abs(own['g_log_alpha']))
        _step_close(_np(agent.log_alpha), _np(la0), np.array([ref['log_alpha']]))
        assert int(agent.temperature.optimizer.iterations.item()) == 1
    else:
        assert agent.log_alpha.cpu().numpy().tobytes() == la0.cpu().numpy().tobytes()
        assert int(agent.temperature.optimizer.iterations.item()) == 0
    for tm, t0, th in zip((agent.target_critic1, agent.target_critic2), tt0, dev_critics):
        np.testing.assert_allclose(_np(tm.theta), (1 - tau) * t0 + tau * th, rtol=0,
                                   atol=2e-6 * max(1, np.abs(t0).max()))


def test_captured_gradient_steps_match_eager(device):
    """Four update_weights(2) calls replay captured phases after their eager and capturing
    passes: actor, critics, targets and log_alpha end bit-identical to all-eager launches, so
    alpha and the Philox counter are read on device inside the captured phases."""
    out = []
    for use_graph in (False, True):
        np.random.seed(0)
        random.seed(0)
        agent = _agent(device, 'Pendulum-v1')
        agent.use_graph = use_graph
        agent.fill_buffers()
        for _ in range(4):
            agent.update_weights(2)
        torch.cuda.synchronize()
        assert (agent._phases['actor'].graph is not None) == use_graph
        assert int(agent.temperature.optimizer.iterations.item()) == 8
        nets = _models(agent) + [agent.target_critic1, agent.target_critic2]
        out.append([m.theta.cpu().numpy() for m in nets] +
                   [agent.log_alpha.cpu().numpy(), agent.rng_counter.cpu().numpy(),
                    agent.eps.cpu().numpy()])
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert out[0][5][0] != np.float32(0.0)  # log_alpha moved from log(1)


def test_train_loop(device):
    """fit() on 4 Pendulum envs with 10-step episodes: episodes end, each triggers a gradient
    step, statistics are reported, every parameter stays finite and alpha positive."""
    agent = _agent(device, 'Pendulum-v1', env_kwargs=dict(max_episode_steps=10),
                   split_critics=False)
    agent.fit(max_steps=4 * 45)
    torch.cuda.synchronize()
    it = int(agent.critic1.optimizer.iterations.item())
    assert it > 0 and it == agent.games
    assert int(agent.actor.optimizer.iterations.item()) == it
    assert int(agent.temperature.optimizer.iterations.item()) == it
    assert len(agent.total_rewards) > 0 and np.isfinite(agent.mean_reward)
    for m in _models(agent) + [agent.target_critic1, agent.target_critic2]:
        assert torch.isfinite(m.theta).all()
    assert np.isfinite(agent.alpha) and agent.alpha > 0
    assert float(agent.step_actions.abs().max()) <= 1.0


def test_play_actions_are_the_mode(device):
    agent = _agent(device, 'BipedalWalker-v3')
    torch.manual_seed(0)
    agent.envs.state.copy_(torch.randn_like(agent.envs.state))
    c0 = int(agent.rng_counter.item())
    play = _np(agent._play_actions())
    mean = _np(agent.ex_step.forward(agent.envs.state)[0])
    torch.cuda.synchronize()
    assert int(agent.rng_counter.item()) == c0  # nothing drawn
    np.testing.assert_allclose(play, np.tanh(mean), rtol=0, atol=ACT_ATOL)
    step = _np(agent.get_step_actions())
    assert int(agent.rng_counter.item()) == c0 + 1 and not np.array_equal(step, play)
    assert np.isfinite(agent.play(max_steps=5))


def test_checkpoint_restores_the_whole_agent(device, tmp_path):
    """checkpoint() then load_weights(): log_alpha, its Adam moments and step count, the
    critics and the targets come back bit for bit, and the next gradient step from the
    restored agent equals the original's (same sample slots, same Philox counter)."""
    def build():
        np.random.seed(0)
        random.seed(0)
        agent = _agent(device, 'Pendulum-v1')
        agent.fill_buffers()
        return agent

    def state(agent):
        opts = [m.optimizer for m in _models(agent)] + [agent.temperature.optimizer]
        ts = [m.theta for m in _models(agent)] + \
            [agent.target_critic1.theta, agent.target_critic2.theta, agent.log_alpha]
        for o in opts:
            ts += [o.m, o.v, o.iterations]
        return [t.cpu().numpy().tobytes() for t in ts]

    a = build()
    a.update_weights(3)
    paths = [str(tmp_path / f'{name}.npz') for name in ('actor', 'critic1', 'critic2')]
    a.checkpoints = paths
    a.mean_reward = 1.0
    a.checkpoint()
    assert a.best_reward == 1.0 and all(Path(p).exists() for p in paths)
    b = build()
    assert state(b) != state(a)
    b.load_weights(paths)
    torch.cuda.synchronize()
    assert state(b) == state(a)
    assert int(b.temperature.optimizer.iterations.item()) == 3
    assert b.temperature.optimizer.m.abs().item() > 0
    b.rng_counter.copy_(a.rng_counter)
    for agent in (a, b):
        np.random.seed(5)
        agent.update_weights(1)
    torch.cuda.synchronize()
    assert state(b) == state(a)
    assert a.s.cpu().numpy().tobytes() == b.s.cpu().numpy().tobytes()
    # a plain model file (no extras) still loads: the target restarts from its model
    a.critic1.save_weights(paths[1])
    b.load_weights(paths)
    assert torch.equal(b.target_critic1.theta, b.critic1.theta)
