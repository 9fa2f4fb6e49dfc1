"""GPU tests of the Pendulum-v1 / MountainCarContinuous-v0 device envs: the step kernel
(xa_continuous_env_step) against the numpy f64 restatement of
tests/test_continuous_envs_host.py, its reset draws, the fused env-step + replay-append launch
against the two-launch composition bit for bit, the continuous-action agents on both forms,
and the step under hipGraph replay.

Bounds (those of the classic step kernel's tests): f64 state within 1e-9 absolute, f32
observations and rewards within 1e-6 of the f32 rounding of the reference's f64 values; done
flags equal. The reference is teacher-forced: at every step it advances one step from the
device's own f64 state. A MountainCarContinuous sample whose reference margin lies within
1e-9 of a threshold (goal line, velocity sign, wall) may legitimately take the other branch
on the device and is left out of the comparison; at most 1 % of the samples may be, and the
reference's own run leaves out none (host test). Pendulum has no discontinuous branch.
"""
import ctypes

import numpy as np
import pytest
import test_continuous_envs_host as ref
import torch

from xagents_amd import _lib

pytestmark = pytest.mark.gpu

PENDULUM, MOUNTAINCAR_CONT = ref.PENDULUM, ref.MOUNTAINCAR_CONT
KINDS = ref.KINDS
ENV_ID = ref.ENV_ID


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device='cuda', dtype=dtype)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def z(*shape, dt=torch.float32):
    return torch.zeros(*shape, dtype=dt, device='cuda')


class RawEnv:
    """The env's own device memory and its launch arguments."""

    def __init__(self, kind, n, seed, limit):
        self.kind, self.n, self.od = kind, n, ref.OBS_DIM[kind]
        self.state64 = z(n, 2, dt=torch.float64)
        self.elapsed, self.episode = z(n, dt=torch.int32), z(n, dt=torch.int32)
        a = _lib.XaContinuousStepArgs()
        a.env_kind, a.n_envs = kind, n
        a.state64, a.elapsed = self.state64.data_ptr(), self.elapsed.data_ptr()
        a.episode, a.seed, a.max_episode_steps = self.episode.data_ptr(), seed, limit
        a.act_ld = 1
        self.a = a

    def call(self, step=None):
        _lib.call('xa_continuous_env_step', ctypes.byref(self.a),
                  None if step is None else ctypes.byref(step), _lib.stream())

    def reset(self):
        post = z(self.n, self.od)
        self.a.reset_only, self.a.out_post = 1, post.data_ptr()
        self.call()
        self.a.reset_only = 0
        return post


# ---- 1. the step kernel against numpy, teacher-forced --------------------------------------
@pytest.mark.parametrize('act_ld', ref.STEP_CASE['act_ld'])
@pytest.mark.parametrize('n', ref.STEP_CASE['n_envs'])
@pytest.mark.parametrize('kind', KINDS)
def test_step_matches_numpy_teacher_forced(device, kind, n, act_ld):
    T, limit, od = ref.STEP_CASE['steps'], ref.STEP_CASE['limit'], ref.OBS_DIM[kind]
    acts, plants = ref.step_case(kind, n)
    env = RawEnv(kind, n, 0xabcdef12345, limit)
    env.reset()
    # strided actions: the env's action is element 0 of its row, the rest is poison
    act_buf = torch.full((T, n, act_ld), 99.0, device='cuda')
    act_buf[:, :, 0] = dev(acts)
    pre_S, post_S = z(T, n, 2, dt=torch.float64), z(T, n, 2, dt=torch.float64)
    pre_E, post_E = z(T, n, dt=torch.int32), z(T, n, dt=torch.int32)
    pre_P, post_P = z(T, n, dt=torch.int32), z(T, n, dt=torch.int32)
    obs, post = z(T, n, od), z(T, n, od)
    rew, done = z(T, n), torch.full((T, n), -1.0, device='cuda')
    a = env.a
    a.act_ld = act_ld
    for t in range(T):
        for pt, e, state, _ in plants:
            if pt == t:
                env.state64[e] = dev(state)
        pre_S[t].copy_(env.state64)
        pre_E[t].copy_(env.elapsed)
        pre_P[t].copy_(env.episode)
        a.actions = act_buf[t].data_ptr()
        a.out_obs, a.out_post = obs[t].data_ptr(), post[t].data_ptr()
        a.out_rew, a.out_done = rew[t].data_ptr(), done[t].data_ptr()
        env.call()
        post_S[t].copy_(env.state64)
        post_E[t].copy_(env.elapsed)
        post_P[t].copy_(env.episode)
    S, nS = host(pre_S).reshape(-1, 2), host(post_S).reshape(-1, 2)
    E, nE = host(pre_E).reshape(-1).astype(np.int64), host(post_E).reshape(-1)
    P, nP = host(pre_P).reshape(-1), host(post_P).reshape(-1)
    obs, post = host(obs).reshape(-1, od), host(post).reshape(-1, od)
    rew, done = host(rew).reshape(-1), host(done).reshape(-1)

    r = ref.ref_step(kind, S, E, acts.reshape(-1), limit)
    near = r['near']
    print(f'kind {kind}: {near.sum()} of {near.size} samples within {ref.NEAR} of a threshold')
    assert near.mean() <= 0.01
    ok = ~near
    assert set(np.unique(done)) <= {0.0, 1.0}
    d_obs = np.abs(obs[ok].astype(np.float64) - r['obs'][ok].astype(np.float64)).max()
    d_rew = np.abs(rew[ok].astype(np.float64) - r['rew'][ok].astype(np.float64)).max()
    cont = ok & ~r['done']  # the episode goes on: the state is the stepped state
    d_state = np.abs(nS[cont] - r['state'][cont]).max()
    print(f'kind {kind} n {n} act_ld {act_ld}: max |obs| diff {d_obs:.3e}, |rew| diff '
          f'{d_rew:.3e}, |state| diff {d_state:.3e}')
    assert np.array_equal(done[ok] != 0, r['done'][ok])
    assert d_obs <= 1e-6 and d_rew <= 1e-6 and d_state <= 1e-9
    assert np.array_equal(nE[cont], r['elapsed'][cont])
    # finished episodes restart inside gym's reset ranges and advance the env's episode counter
    fin = done != 0
    assert fin.any() and (nE[fin] == 0).all() and ref.reset_in_range(kind, nS[fin]).all()
    assert np.array_equal(nP, P + fin)
    # the post-step record is the observation of the state carried on (the reset when done)
    assert np.abs(post.astype(np.float64) - ref.observe(kind, nS).astype(np.float64)).max() <= 1e-6
    for name in ref.STEP_EVENTS[kind]:
        assert (r['events'][name] & ok).any(), f'branch {name} never fired'
    if kind == MOUNTAINCAR_CONT:
        wall, goal = ok & r['events']['wall'], ok & r['events']['goal']
        assert (nS[wall & ~fin, 0] == -1.2).all() and (nS[wall & ~fin, 1] == 0.0).all()
        a64 = acts.reshape(-1).astype(np.float64)
        # 100 - 0.1 a^2 in f32: half an ulp at [64, 128) is 2^-18
        assert np.abs(rew[goal] - (100.0 - 0.1 * a64[goal] ** 2)).max() <= 2.0 ** -18
        assert (done[goal] == 1.0).all()
    else:
        assert (np.abs(S[:, 0]) > np.pi).any() and (np.abs(nS[:, 1]) <= 8.0).all()


# ---- 2. resets -----------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_reset_draws(device, kind):
    n = 37

    def episodes(seed, count=4):
        """The reset states of `count` successive episodes (TimeLimit 1: every step ends
        one), the first from reset_only called twice."""
        env = RawEnv(kind, n, seed, 1)
        env.state64.fill_(123.0)
        env.elapsed.fill_(7)
        post = env.reset()
        out = [host(env.state64).copy()]
        assert (host(env.elapsed) == 0).all() and (host(env.episode) == 0).all()
        assert np.abs(host(post).astype(np.float64)
                      - ref.observe(kind, out[0]).astype(np.float64)).max() <= 1e-6
        env.reset()
        assert np.array_equal(host(env.state64), out[0])  # no step in between: the same draw
        acts = z(n)
        rec = [z(n, env.od), z(n, env.od), z(n), z(n)]
        a = env.a
        a.actions = acts.data_ptr()
        a.out_obs, a.out_post, a.out_rew, a.out_done = (t.data_ptr() for t in rec)
        for k in range(1, count):
            env.call()
            assert (host(rec[3]) == 1.0).all() and (host(env.episode) == k).all()
            out.append(host(env.state64).copy())
        return out

    first = episodes(77)
    for s in first:
        assert ref.reset_in_range(kind, s).all()
        assert len(np.unique(s[:, 0])) == n  # every env its own draw
    for s0, s1 in zip(first, first[1:]):
        assert (s0[:, 0] != s1[:, 0]).all()  # an env's successive episodes differ
    again, other = episodes(77), episodes(78)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    assert all((x[:, 0] != y[:, 0]).all() for x, y in zip(first, other))


@pytest.mark.parametrize('kind', KINDS)
def test_env_object_reset_and_surface(device, kind):
    from xagents_amd.envs import Box, ContinuousControlVecEnv, create_envs
    env = create_envs(ENV_ID[kind], 6, device=device, seed=5)
    assert type(env) is ContinuousControlVecEnv and not env.has_pre_step and env.fused
    for mode in ('dynamics', 'transitions'):
        assert type(create_envs(ENV_ID[kind], 2, device=device, mode=mode)) is type(env)
    assert env.spec.max_episode_steps == env.max_episode_steps == ref.TIME_LIMIT[kind]
    assert isinstance(env.action_space, Box) and env.action_space.shape == (1,)
    assert env.action_space.high == ref.ACTION_BOUND[kind] == -env.action_space.low
    assert env.observation_space.shape == (ref.OBS_DIM[kind],)
    s0, o0 = host(env.state64).copy(), host(env.state).copy()
    assert ref.reset_in_range(kind, s0).all()
    assert np.abs(o0.astype(np.float64) - ref.observe(kind, s0).astype(np.float64)).max() <= 1e-6
    env.reset()
    assert np.array_equal(host(env.state64), s0) and np.array_equal(host(env.state), o0)
    composed = create_envs(ENV_ID[kind], 6, device=device, seed=5, fused=False,
                           max_episode_steps=9)
    assert composed.has_pre_step and composed.max_episode_steps == 9
    assert np.array_equal(host(composed.state64), s0)


# ---- 3. the fused launch equals env step + xa_replay_env_step, bit for bit -----------------
class StepSide:
    """One side of the comparison: an env, the agent-side arrays and (optionally) a ring."""

    def __init__(self, kind, n, cap, ring_kind, out_ld, seed, limit):
        self.env = env = RawEnv(kind, n, seed, limit)
        od = env.od
        post = env.reset()
        ld = max(out_ld, 1)
        self.arrays = dict(
            state=post.clone(), ep_return=z(n), done=z(n),
            cursor=torch.full((n,), 0, dtype=torch.int32, device='cuda'),
            out_states=torch.full((n, od), -7.0, device='cuda'),
            out_new_states=torch.full((n, od), -7.0, device='cuda'),
            out_rewards=torch.full((n, ld), -7.0, device='cuda'),
            out_dones=torch.full((n, ld), -7.0, device='cuda'),
            done_epret=torch.full((n, ld), -7.0, device='cuda'))
        if ring_kind is not None:
            self.arrays.update(
                ring_states=torch.full((n, cap, od), -7.0, device='cuda'),
                ring_new_states=torch.full((n, cap, od), -7.0, device='cuda'),
                ring_actions=torch.full((n, cap, 1), -7.0, device='cuda'),
                ring_rewards=torch.full((n, cap), -7.0, device='cuda'),
                ring_dones=torch.full((n, cap), -7.0, device='cuda'),
                ring_count=z(n, dt=torch.int64))
        r = _lib.XaReplayStepArgs()
        r.n_envs, r.obs_bytes, r.out_ld = n, 4 * od, out_ld
        for name, t in self.arrays.items():
            setattr(r, name, t.data_ptr())
        if ring_kind is not None:
            r.capacity, r.ring_kind, r.act_bytes = cap, ring_kind, 4
        self.r = r

    def snapshot(self):
        out = {k: host(t).copy() for k, t in self.arrays.items()}
        out.update(state64=host(self.env.state64).copy(), elapsed=host(self.env.elapsed).copy(),
                   episode=host(self.env.episode).copy())
        return out


# both ring kinds at both output strides, and once without a ring (ring_states = NULL)
RING_CASES = [(_lib.XA_RING_DEQUE, 0), (_lib.XA_RING_DEQUE, 10), (_lib.XA_RING_RB2, 0),
              (_lib.XA_RING_RB2, 10), (None, 0)]


@pytest.mark.parametrize('ring_kind,out_ld', RING_CASES)
@pytest.mark.parametrize('kind', KINDS)
def test_fused_step_equals_composed_bit_for_bit(device, kind, ring_kind, out_ld):
    n, cap, steps, limit, od = 5, 4, 12, 3, ref.OBS_DIM[kind]
    rng = np.random.default_rng(31 + kind)
    bound = ref.ACTION_BOUND[kind]
    acts = rng.uniform(-1.5 * bound, 1.5 * bound, (steps, n, 1)).astype(np.float32)
    fused = StepSide(kind, n, cap, ring_kind, out_ld, 99, limit)
    comp = StepSide(kind, n, cap, ring_kind, out_ld, 99, limit)
    # the fused launch ignores the recorded stream and the cursor: leave them NULL / marked
    fused.arrays['cursor'].fill_(123)
    fused.r.t_rec = 0
    rec = [z(n, 1, od), z(n, 1, od), z(n, 1), z(n, 1)]
    c = comp.r
    c.t_rec = 1
    c.rep_obs, c.rep_state, c.rep_rew, c.rep_done = (t.data_ptr() for t in rec)
    a = comp.env.a
    a.out_obs, a.out_post, a.out_rew, a.out_done = c.rep_obs, c.rep_state, c.rep_rew, c.rep_done
    dones = 0
    for t in range(steps):
        act = dev(acts[t])
        for side in (fused, comp):
            side.env.a.actions = act.data_ptr()
            side.r.actions = act.data_ptr()
        fused.env.call(fused.r)
        comp.env.call()
        _lib.call('xa_replay_env_step', ctypes.byref(c), _lib.stream())
        f, g = fused.snapshot(), comp.snapshot()
        assert (f.pop('cursor') == 123).all() and (g.pop('cursor') == 0).all()
        for name in g:
            assert f[name].tobytes() == g[name].tobytes(), f'{name} differs at step {t}'
        dones += int(g['done'].sum())
        # the rows are what the step says: state <- post-step observation, strided outputs
        assert np.array_equal(g['out_rewards'][:, 1:], np.full((n, max(out_ld, 1) - 1), -7.0,
                                                               np.float32))
        assert np.abs(g['state'].astype(np.float64)
                      - ref.observe(kind, g['state64']).astype(np.float64)).max() <= 1e-6
    assert dones == n * (steps // limit)
    if ring_kind is not None:
        want = np.full(n, cap if ring_kind == _lib.XA_RING_RB2 else steps)
        assert np.array_equal(g['ring_count'], want)  # the ring wrapped / RB2 saturated
        assert (g['ring_states'] != -7.0).all()
        if ring_kind == _lib.XA_RING_DEQUE:
            # slot (t % cap) of env i holds step t's action
            last = acts[steps - cap:, :, 0].T
            assert np.array_equal(g['ring_actions'][:, :, 0], np.roll(last, steps % cap, 1))


# ---- 4. the agents -------------------------------------------------------------------------
def _offpolicy_agent(algo, env_id, fused, device, n=4, limit=6):
    from xagents_amd import DDPG, TD3
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    envs = create_envs(env_id, n, device=device, seed=4, max_episode_steps=limit, fused=fused)
    kw = dict(seed=7, device=device)
    actor = create_model(envs, algo, 'actor_model', **kw)
    critic = create_model(envs, algo, 'critic_model', **kw)
    bufs = create_buffers(algo, 16 * n, 2 * n, n, initial_size=4 * n)
    return (TD3 if algo == 'td3' else DDPG)(envs, actor, critic, bufs, seed=3, quiet=True,
                                            gradient_steps=1)


def _offpolicy_run(algo, env_id, fused, device):
    agent = _offpolicy_agent(algo, env_id, fused, device)
    agent.fill_buffers()
    for _ in range(12):
        agent.train_step()
    agent._drain_episode_stats()
    models = [agent.actor, agent.critic, agent.target_actor, agent.target_critic]
    models += [getattr(agent, m) for m in ('critic2', 'target_critic2') if hasattr(agent, m)]
    rep = agent.replay
    out = dict(theta=[host(m.theta).copy() for m in models],
               rings=[host(t).copy() for t in (rep.states, rep.new_states, rep.actions,
                                               rep.rewards, rep.dones, rep.count)],
               total_rewards=list(agent.total_rewards), steps=agent.steps,
               state64=host(agent.envs.state64).copy())
    return agent, out


@pytest.mark.parametrize('algo,env_id', [('td3', 'Pendulum-v1'), ('ddpg', 'Pendulum-v1'),
                                         ('td3', 'MountainCarContinuous-v0')])
def test_td3_ddpg_train_identically_on_both_env_forms(device, algo, env_id):
    agent, got = _offpolicy_run(algo, env_id, True, device)
    # the fused env took the staged env phase of train_step, the composed one the eager path
    assert hasattr(agent, '_stage') and agent.envs.has_pre_step is False
    ref_agent, want = _offpolicy_run(algo, env_id, False, device)
    assert not hasattr(ref_agent, '_stage') and ref_agent.envs.has_pre_step is True
    assert got['steps'] == want['steps'] == 12 * 4
    for x, y in zip(got['theta'], want['theta']):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()
    for x, y in zip(got['rings'], want['rings']):
        assert x.tobytes() == y.tobytes()
    assert got['state64'].tobytes() == want['state64'].tobytes()
    assert got['total_rewards'] == want['total_rewards'] and len(got['total_rewards']) == 8
    # gradient steps fired: the online actor left its initial weights (the target's start)
    fresh = _offpolicy_agent(algo, env_id, True, device)
    assert not np.array_equal(got['theta'][0], host(fresh.actor.theta))
    for ag in (agent, ref_agent):
        total = ag.play(max_steps=9)
        assert np.isfinite(total)
    if env_id == 'Pendulum-v1':
        assert total < 0.0  # Pendulum's reward is a negated cost


def test_gaussian_ppo_trains_identically_on_both_env_forms(device):
    from xagents_amd import PPO
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_model
    thetas = []
    for fused in (True, False):
        envs = create_envs('Pendulum-v1', 4, device=device, seed=9, max_episode_steps=6,
                           fused=fused)
        model = create_model(envs, 'ppo', 'model', seed=3, device=device)
        agent = PPO(envs, model, n_steps=8, seed=8, quiet=True, ppo_epochs=1, mini_batches=2)
        assert agent.executor_path and agent.gaussian
        theta0 = host(model.theta).copy()
        agent.train_step()
        agent.train_step()
        theta = host(model.theta).copy()
        assert np.isfinite(theta).all() and not np.array_equal(theta, theta0)
        assert host(agent.b_done).sum() > 0  # the TimeLimit ended episodes inside the rollout
        thetas.append((theta, host(envs.state64).copy(), host(agent.b_rew).copy()))
        assert np.isfinite(agent.play(max_steps=9))
    for x, y in zip(*thetas):
        assert x.tobytes() == y.tobytes()


# ---- 5. the env phase under hipGraph replay ------------------------------------------------
def test_captured_step_draws_fresh_resets(device, monkeypatch):
    """The reset draw is keyed by the env's own episode counter in device memory: a
    captured env phase must draw a new initial state at every episode boundary it replays."""
    monkeypatch.setenv('XA_TD3_STEP_GRAPH', '1')
    limit, n = 3, 4
    agent = _offpolicy_agent('td3', 'Pendulum-v1', True, device, n=n, limit=limit)
    agent.fill_buffers()
    envs = agent.envs
    ep0 = host(envs.episode).copy()
    resets = []
    for t in range(4 * limit):
        agent.train_step()
        if (t + 1) % limit == 0:
            assert (host(envs.elapsed) == 0).all()
            resets.append(host(envs.state64).copy())
    assert agent._step_graph and agent._phases['step'].graph is not None
    assert np.array_equal(host(envs.episode), ep0 + 4)
    for s in resets:
        assert ref.reset_in_range(PENDULUM, s).all()
    # boundaries 2..4 were drawn by graph replays
    for s0, s1 in zip(resets, resets[1:]):
        assert (s0[:, 0] != s1[:, 0]).all()
    assert np.abs(host(envs.state).astype(np.float64)
                  - ref.observe(PENDULUM, resets[-1]).astype(np.float64)).max() <= 1e-6
