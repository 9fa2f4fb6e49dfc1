"""The A/B knobs that choose how host-drawn sample slots reach the launch that reads them
(XA_PINNED_SLOTS, XA_TD3_STAGED_SLOTS) and where the TD3 step's statistics row lands
(XA_TD3_HOST_STAGE) change the transport only: an agent run with a knob on and one run with it
off, from the same seeds, end with the same bytes in every model's parameters and Adam state
and the same episode statistics. And a staged buffer is not overwritten before its launch read
it: each fused gradient step gathers the batch of its own slot vector."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 6


def _seed_host(s):
    np.random.seed(s)
    random.seed(s)


def _dqn(device):
    from xagents_amd import DQN
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    envs = create_envs('PongNoFrameskip-v4', 2, device=device, seed=3)
    model = create_model(envs, 'dqn', 'model', seed=9, device=device)
    return DQN(envs, model, create_buffers('dqn', 40, 4, 2, initial_size=20), seed=2,
               quiet=True, epsilon_decay_steps=20, target_sync_steps=3)


def _td3(device):
    from xagents_amd import TD3
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    n = 4
    envs = create_envs('BipedalWalker-v3', n, mode='dynamics', device=device, seed=4)
    kw = dict(seed=7, device=device, optimizer_kwargs=dict(learning_rate=1e-3))
    actor = create_model(envs, 'td3', 'actor_model', **kw)
    critic = create_model(envs, 'td3', 'critic_model', **kw)
    bufs = create_buffers('td3', 64 * n, 2 * n, n, initial_size=8 * n)
    return TD3(envs, actor, critic, bufs, seed=3, quiet=True, gradient_steps=1)


def _state(agent):
    """{name: bytes} of every model's theta and Adam m / v / iterations, plus the episode
    statistics."""
    agent._drain_episode_stats()
    torch.cuda.synchronize()
    out, seen = {}, set()
    for name, m in sorted(vars(agent).items()):
        if hasattr(m, 'theta') and hasattr(m, 'optimizer') and id(m) not in seen:
            seen.add(id(m))
            out[f'{name}.theta'] = m.theta.cpu().numpy().tobytes()
            for k in ('m', 'v', 'iterations'):
                t = getattr(m.optimizer, k, None)
                if isinstance(t, torch.Tensor):
                    out[f'{name}.{k}'] = t.cpu().numpy().tobytes()
    out['total_rewards'] = list(agent.total_rewards)
    out['games'] = agent.games
    return out


def _run(make, device, monkeypatch, env, extra_updates=0):
    """STEPS train steps (and `extra_updates` more gradient steps) of a freshly built agent
    under the XA_* settings `env`; its end state."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    _seed_host(4)
    agent = make(device)
    agent.fill_buffers()
    for _ in range(STEPS):
        agent.at_step_start()
        agent.train_step()
        agent.at_step_end()
    if extra_updates:
        agent.update_weights(extra_updates)
    return agent, _state(agent)


def _assert_same(on, off):
    assert on.keys() == off.keys() and any(k.endswith('.iterations') for k in on)
    for k in on:
        assert on[k] == off[k], k


@pytest.mark.parametrize('learn_graph', ['0', '1'])
def test_dqn_staged_slots_equal_uploaded(device, monkeypatch, learn_graph):
    """XA_PINNED_SLOTS 1 (the gather reads mapped pinned memory) against 0 (upload copy)."""
    res = {}
    for knob in ('1', '0'):
        agent, res[knob] = _run(_dqn, device, monkeypatch,
                                {'XA_PINNED_SLOTS': knob, 'XA_DQN_LEARN_GRAPH': learn_graph})
        assert int(agent.model.optimizer.iterations.item()) == STEPS
        assert (agent._lgraph is not None) == (learn_graph == '1')
    _assert_same(res['1'], res['0'])


@pytest.mark.parametrize('graph', ['0', '1'])
def test_td3_staged_slots_equal_uploaded(device, monkeypatch, graph):
    """XA_TD3_STAGED_SLOTS 1 against 0; the odd number of extra gradient steps makes both
    rotating buffers (and, replayed, both buffers' captured graphs) run."""
    res = {}
    for knob in ('1', '0'):
        agent, res[knob] = _run(_td3, device, monkeypatch,
                                {'XA_TD3_STAGED_SLOTS': knob, 'XA_TD3_GRAPH': graph}, 5)
        assert agent._fused_args() is not None  # the one-launch step reads the slots
        assert int(agent.critic1.optimizer.iterations.item()) >= 5
    _assert_same(res['1'], res['0'])


def test_td3_host_stage_equals_device_stage(device, monkeypatch):
    """XA_TD3_HOST_STAGE 1 (the step's statistics row stored into mapped host memory) against
    0 (a device row, copied back)."""
    res = {knob: _run(_td3, device, monkeypatch, {'XA_TD3_HOST_STAGE': knob}, 5)[1]
           for knob in ('1', '0')}
    _assert_same(res['1'], res['0'])


def test_td3_staged_buffer_not_overwritten_before_read(device, monkeypatch):
    """Three fused gradient steps enqueued back to back, each with its own slot vector (the
    third reuses the first's buffer): every step's gathered batch is the rings at ITS vector.
    The batches are copied on the stream between the steps, without a host wait."""
    monkeypatch.setenv('XA_TD3_STAGED_SLOTS', '1')
    _seed_host(4)
    agent = _td3(device)
    agent.fill_buffers()
    assert agent._fused_args() is not None
    r = agent.replay
    filled = int(r.host_count.min())
    base = np.repeat(np.arange(r.n, dtype=np.int64) * r.cap, r.k)
    rng = np.random.default_rng(5)
    vectors = [base + rng.integers(0, filled, r.n * r.k) for _ in range(3)]
    assert all((vectors[i] != vectors[j]).any() for i in range(3) for j in range(i))
    fields = ('s', 'a', 'r', 'd', 's2')
    seen, calls = [], []

    def snapshot():
        seen.append([getattr(agent, f).clone() for f in fields])

    def sample_slots():
        if calls:
            snapshot()  # the previous step's batch, behind its launch on the stream
        calls.append(1)
        return vectors[len(calls) - 1]

    monkeypatch.setattr(r, 'sample_slots', sample_slots)
    agent.update_weights(3)
    snapshot()
    torch.cuda.synchronize()
    assert len(calls) == 3 and len(seen) == 3
    rings = (r.states, r.actions, r.rewards, r.dones, r.new_states)
    for step, (vec, got) in enumerate(zip(vectors, seen)):
        idx = torch.from_numpy(vec).to(device)
        for f, ring, t in zip(fields, rings, got):
            want = ring.reshape((r.n * r.cap,) + ring.shape[2:])[idx].reshape(t.shape)
            assert torch.equal(t, want), (step, f)
