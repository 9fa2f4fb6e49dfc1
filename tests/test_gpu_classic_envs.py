"""GPU tests of the Acrobot-v1 / MountainCar-v0 device envs: the step kernel
(xa_classic_step) against the numpy f64 restatement of tests/test_classic_envs_host.py, the
fused rollout against the step kernel bit for bit, and the agents on both paths.

Bounds (those of test_rollout_cartpole_dynamics): f64 state within 1e-9 absolute, f32
observations and rewards within 1e-6; done flags equal. The reference is teacher-forced: at
every step it advances one step from the device's own f64 state. A sample whose reference
margin lies within 1e-9 of a threshold (the Acrobot terminal line; MountainCar's goal line,
velocity sign and wall) may legitimately take the other branch on the device, so it is left
out of the comparison of the done flag and of what that branch decides (reward, state); at
most 1 % of the samples may be left out, and the reference's own run leaves out none (host
test).
"""
import ctypes

import numpy as np
import pytest
import test_classic_envs_host as ref
import torch

from xagents_amd import _lib, kernels

pytestmark = pytest.mark.gpu

ACROBOT, MOUNTAINCAR = ref.ACROBOT, ref.MOUNTAINCAR
KINDS = [ACROBOT, MOUNTAINCAR]
ENV_ID = {ACROBOT: 'Acrobot-v1', MOUNTAINCAR: 'MountainCar-v0'}


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device='cuda', dtype=dtype)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _step_args(kind, n, state64, elapsed, seed, counter, limit):
    a = _lib.XaClassicStepArgs()
    a.env_kind, a.n_envs = kind, n
    a.state64, a.elapsed = state64.data_ptr(), elapsed.data_ptr()
    a.seed, a.counter, a.max_episode_steps = seed, counter.data_ptr(), limit
    return a


def _check_against_reference(kind, S, E, acts, obs, post, rew, done, limit):
    """S [T + 1, n, 4] / E [T + 1, n]: the device's state and elapsed count before every
    step (and after the last); obs / post / rew / done [T, n, ...]: its step records. All
    steps at once: the reference steps every (t, env) sample from S[t]."""
    T, n = acts.shape
    od = ref.OBS_DIM[kind]
    r = ref.ref_step(kind, S[:-1].reshape(-1, 4), E[:-1].reshape(-1).astype(np.int64),
                     acts.reshape(-1), limit)
    near = r['near']
    print(f'kind {kind}: {near.sum()} of {near.size} samples within {ref.NEAR} of a threshold')
    assert near.mean() <= 0.01
    ok = ~near
    nS, nE = S[1:].reshape(-1, 4), E[1:].reshape(-1)
    obs, post = obs.reshape(-1, od), post.reshape(-1, od)
    rew, done = rew.reshape(-1), done.reshape(-1)
    assert set(np.unique(done)) <= {0.0, 1.0}
    d_obs = np.abs(obs[ok].astype(np.float64) - r['obs'][ok]).max()
    d_rew = np.abs(rew[ok].astype(np.float64) - r['rew'][ok]).max()
    cont = ok & ~r['done']  # the episode goes on: the state is the stepped state
    d_state = np.abs(nS[cont] - r['state'][cont]).max()
    print(f'kind {kind}: max |obs| diff {d_obs:.3e}, |rew| diff {d_rew:.3e}, '
          f'|state| diff {d_state:.3e}')
    assert np.array_equal(done[ok] != 0, r['done'][ok])
    assert d_obs <= 1e-6 and d_rew <= 1e-6 and d_state <= 1e-9
    assert np.array_equal(nE[cont], r['elapsed'][cont])
    # finished episodes restart inside gym's reset ranges (MountainCar at rest)
    fin = done != 0
    assert fin.any() and (nE[fin] == 0).all() and ref.reset_in_range(kind, nS[fin]).all()
    if kind == MOUNTAINCAR:
        # slots 2 and 3 are not MountainCar's: untouched; the wall leaves v = 0 exactly
        assert np.array_equal(nS[:, 2:], S[:-1].reshape(-1, 4)[:, 2:])
        wall = ok & r['events']['wall']
        assert (nS[wall, 0] == -1.2).all() and (nS[wall, 1] == 0.0).all()
    # the post-step record is the observation of the state carried on (the reset when done)
    assert np.abs(post.astype(np.float64) - ref.observe(kind, nS)).max() <= 1e-6
    for name in ref.STEP_EVENTS[kind]:
        assert (r['events'][name] & ok).any(), f'branch {name} never fired'
    return r


# ---- (a) the step kernel against numpy, teacher-forced -------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_classic_step_matches_numpy_teacher_forced(device, kind):
    n, T = ref.STEP_CASE['n'], ref.STEP_CASE['steps']
    limit = ref.STEP_CASE['limit'][kind]
    od = ref.OBS_DIM[kind]
    s0, acts = ref.step_case(kind)
    if kind == MOUNTAINCAR:
        s0[:, 2:] = [3.25, -7.5]  # not MountainCar's slots: must come back untouched
    state, elapsed = dev(s0), torch.zeros(n, dtype=torch.int32, device='cuda')
    counter = torch.tensor([5], dtype=torch.int64, device='cuda')
    # strided actions: the env's action is element 0 of its row of 3, the rest is poison
    act_buf = torch.full((T, n, 3), 99, dtype=torch.int32, device='cuda')
    act_buf[:, :, 0] = dev(acts)
    S = torch.zeros(T + 1, n, 4, dtype=torch.float64, device='cuda')
    E = torch.zeros(T + 1, n, dtype=torch.int32, device='cuda')
    obs, post = torch.zeros(T, n, od, device='cuda'), torch.zeros(T, n, od, device='cuda')
    rew, done = torch.zeros(T, n, device='cuda'), torch.full((T, n), -1.0, device='cuda')
    a = _step_args(kind, n, state, elapsed, 0xabcdef12345, counter, limit)
    a.act_ld = 3
    S[0].copy_(state)
    for t in range(T):
        a.actions, a.t = act_buf[t].data_ptr(), t
        a.out_obs, a.out_post = obs[t].data_ptr(), post[t].data_ptr()
        a.out_rew, a.out_done = rew[t].data_ptr(), done[t].data_ptr()
        _lib.call('xa_classic_step', ctypes.byref(a), _lib.stream())
        S[t + 1].copy_(state)
        E[t + 1].copy_(elapsed)
    _check_against_reference(kind, host(S), host(E), acts, host(obs), host(post), host(rew),
                             host(done), limit)


@pytest.mark.parametrize('kind', KINDS)
def test_classic_step_reset_only_and_action_clamp(device, kind):
    """reset_only draws every env inside gym's reset range (the same draw for the same key,
    another for another step index); actions outside [0, 3) act as the nearest valid one on
    the device, and the env's pre_step refuses them on the host."""
    from xagents_amd.envs import ClassicControlVecEnv
    n, od = 37, ref.OBS_DIM[kind]
    counter = torch.tensor([9], dtype=torch.int64, device='cuda')
    draws = []
    for t in (-1, -1, 4):
        state = torch.full((n, 4), 123.0, dtype=torch.float64, device='cuda')
        elapsed = torch.full((n,), 7, dtype=torch.int32, device='cuda')
        post = torch.zeros(n, od, device='cuda')
        a = _step_args(kind, n, state, elapsed, 77, counter, 50)
        a.reset_only, a.t, a.out_post = 1, t, post.data_ptr()
        _lib.call('xa_classic_step', ctypes.byref(a), _lib.stream())
        s = host(state)
        if kind == MOUNTAINCAR:
            assert (s[:, 2:] == 123.0).all()
            s[:, 2:] = 0.0
        assert ref.reset_in_range(kind, s).all() and (host(elapsed) == 0).all()
        assert np.abs(host(post).astype(np.float64) - ref.observe(kind, s)).max() <= 1e-6
        draws.append(s)
    assert np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[0], draws[2])
    assert len(np.unique(draws[0][:, 0])) == n  # every env its own draw

    def step(actions):
        state, elapsed = dev(draws[0]), torch.zeros(n, dtype=torch.int32, device='cuda')
        out = [torch.zeros(n, od, device='cuda'), torch.zeros(n, od, device='cuda'),
               torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')]
        acts = dev(np.asarray(actions, np.int32))
        a = _step_args(kind, n, state, elapsed, 77, counter, 50)
        a.actions, a.act_ld = acts.data_ptr(), 1
        a.out_obs, a.out_post, a.out_rew, a.out_done = (o.data_ptr() for o in out)
        _lib.call('xa_classic_step', ctypes.byref(a), _lib.stream())
        return host(state)

    wild = np.where(np.arange(n) % 2 == 0, -5, 7)
    assert np.array_equal(step(wild), step(np.clip(wild, 0, 2)))
    assert not np.array_equal(step(np.zeros(n)), step(np.full(n, 2)))
    env = ClassicControlVecEnv(ENV_ID[kind], 5, seed=3, device='cuda')
    with pytest.raises(ValueError, match=r'\[0, 3\)'):
        env.pre_step(dev(np.int32([0, 1, 2, 3, 0])))


# ---- (b) the fused rollout equals the step kernel bit for bit ------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_fused_rollout_equals_step_kernel_bit_for_bit(device, kind):
    n, T, limit = 16, 70, 25  # 70 steps: one 64-step chunk and a tail
    od, seed = ref.OBS_DIM[kind], 0x5eed0000 + kind
    rng = np.random.default_rng(40 + kind)
    s0 = ref.wide_start(kind, n, rng)
    theta = dev((rng.standard_normal(kernels.mlp_param_count(od, 3)) * 0.3).astype(np.float32))
    counter = torch.tensor([7], dtype=torch.int64, device='cuda')
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device='cuda')  # noqa: E731
    env_state, env_state64 = dev(ref.observe(kind, s0)), dev(s0)
    env_done, cursor, ep_ret = z(n), z(n, dt=torch.int32), z(n)
    b = dict(obs=z(n, T, od), act=z(n, T, dt=torch.int32), logp=z(n, T), val=z(n, T),
             ent=z(n, T), rew=z(n, T), done=z(n, T + 1), epret=z(n, T), next_val=z(n))
    a = _lib.XaRolloutArgs()
    a.n_envs, a.n_steps, a.obs_dim, a.n_actions = n, T, od, 3
    a.theta, a.env_kind = theta.data_ptr(), kind
    a.env_state, a.env_state64 = env_state.data_ptr(), env_state64.data_ptr()
    a.env_done, a.env_cursor, a.ep_return = env_done.data_ptr(), cursor.data_ptr(), \
        ep_ret.data_ptr()
    a.max_episode_steps = limit
    a.uniforms, a.seed, a.rng_counter = None, seed, counter.data_ptr()
    a.obs_out, a.act_out, a.logp_out = b['obs'].data_ptr(), b['act'].data_ptr(), \
        b['logp'].data_ptr()
    a.val_out, a.ent_out, a.rew_out = b['val'].data_ptr(), b['ent'].data_ptr(), \
        b['rew'].data_ptr()
    a.done_out, a.epret_out, a.next_val = b['done'].data_ptr(), b['epret'].data_ptr(), \
        b['next_val'].data_ptr()
    a.ret_out, a.return_kind = None, 0
    kernels.rollout(a)

    # the same actions, one step kernel launch per step (column t of act_out, stride T)
    state, elapsed = dev(s0), z(n, dt=torch.int32)
    obs, post, rew, done = z(T, n, od), z(T, n, od), z(T, n), z(T, n)
    c = _step_args(kind, n, state, elapsed, seed, counter, limit)
    c.act_ld = T
    for t in range(T):
        c.actions, c.t = b['act'].data_ptr() + 4 * t, t
        c.out_obs, c.out_post = obs[t].data_ptr(), post[t].data_ptr()
        c.out_rew, c.out_done = rew[t].data_ptr(), done[t].data_ptr()
        _lib.call('xa_classic_step', ctypes.byref(c), _lib.stream())

    r_obs, r_done, acts = host(b['obs']), host(b['done']), host(b['act'])
    # obs_out[:, t] is the policy input of step t: the carried-in state, then the pre-reset
    # observation returned by step t - 1
    assert np.array_equal(r_obs[:, 0], ref.observe(kind, s0))
    assert np.array_equal(r_obs[:, 1:], host(obs).transpose(1, 0, 2)[:, :-1])
    assert np.array_equal(host(b['rew']), host(rew).T)
    assert np.array_equal(r_done[:, 1:], host(done).T) and (r_done[:, 0] == 0).all()
    assert np.array_equal(host(env_state64), host(state))
    assert np.array_equal(host(env_state), host(post)[-1])
    assert np.array_equal(host(cursor), host(elapsed))
    assert r_done[:, 1:].sum() > 0 and set(np.unique(acts)) == {0, 1, 2}
    assert np.isfinite(host(b['val'])).all() and np.isfinite(host(b['logp'])).all()
    # the rows are gym's: reward -1 (Acrobot: 0 on a terminal step), running episode returns
    want = {-1.0, 0.0} if kind == ACROBOT else {-1.0}
    assert set(np.unique(host(b['rew']))) <= want


# ---- (c) PPO and A2C on the fused path -----------------------------------------------------
@pytest.mark.parametrize('algo', ['ppo', 'a2c'])
@pytest.mark.parametrize('kind', KINDS)
def test_ppo_a2c_train_and_play_on_the_fused_envs(device, kind, algo):
    from xagents_amd import A2C, PPO
    from xagents_amd.envs import AcrobotVecEnv, MountainCarVecEnv, create_envs
    from xagents_amd.utils.common import create_model
    envs = create_envs(ENV_ID[kind], 8, device=device, seed=3)
    assert type(envs) is (AcrobotVecEnv if kind == ACROBOT else MountainCarVecEnv)
    assert type(create_envs(ENV_ID[kind], 8, device=device, seed=3, mode='dynamics')) is \
        type(envs)
    limit = ref.TIME_LIMIT[kind]
    assert envs.max_episode_steps == limit and envs.action_space.n == 3
    assert envs.observation_space.shape == (ref.OBS_DIM[kind],)
    assert ref.reset_in_range(kind, host(envs.state64)).all()
    model = create_model(envs, algo, 'model', seed=3, device=device)
    agent = (PPO if algo == 'ppo' else A2C)(envs, model, n_steps=16, seed=3, quiet=True)
    assert not agent.executor_path
    theta0 = host(model.theta).copy()
    agent.train_step()
    agent.train_step()
    theta = host(model.theta)
    assert np.isfinite(theta).all() and not np.array_equal(theta, theta0)
    # one game of env 0: the total is the sum of its rollout rows up to its first done
    rows = []
    chunk = agent._play_chunk

    def recording_chunk():
        rew, done = chunk()
        rows.append((np.array(rew), np.array(done)))
        return rew, done

    agent._play_chunk = recording_chunk
    total = agent.play()
    rew = np.concatenate([r for r, _ in rows])
    done = np.concatenate([d for _, d in rows])
    k = int(np.nonzero(done)[0][0])
    assert k >= len(rew) - 16  # play stopped in the chunk of env 0's first done
    assert total == float(rew[:k + 1].astype(np.float64).sum())
    assert k + 1 <= limit
    # reward -1 per step; only Acrobot's terminal step (never the TimeLimit's) gives 0
    assert (rew[:k] == -1.0).all() and rew[k] in ((-1.0,) if kind == MOUNTAINCAR else (-1.0, 0.0))

# ---- (d) TRPO on the step-kernel env --------------------------------------------------------
def test_trpo_on_the_acrobot_transition_env(device):
    from xagents_amd import TRPO
    from xagents_amd.envs import ClassicControlVecEnv, create_envs
    from xagents_amd.utils.common import create_model
    n, T = 6, 16
    envs = create_envs('Acrobot-v1', n, mode='transitions', device=device, seed=11)
    assert type(envs) is ClassicControlVecEnv
    s_first = host(envs.state64).copy()
    assert ref.reset_in_range(ACROBOT, s_first).all()
    assert np.abs(host(envs.state).astype(np.float64) - ref.observe(ACROBOT, s_first)).max() <= 1e-6
    actor = create_model(envs, 'trpo', 'actor_model', seed=11, device=device)
    critic = create_model(envs, 'trpo', 'critic_model', seed=12, device=device)
    agent = TRPO(envs, actor, critic, n_steps=T, seed=11, quiet=True)
    # the first train step's rollout runs eagerly: record the env's f64 state before every
    # step, to teacher-force the reference
    snaps = []
    pre_step = envs.pre_step

    def recording_pre_step(actions=None, act_ld=1):
        snaps.append((envs.state64.clone(), envs.elapsed.clone()))
        return pre_step(actions, act_ld)

    envs.pre_step = recording_pre_step
    agent.train_step()
    del envs.pre_step
    assert len(snaps) == T
    S = np.stack([host(s) for s, _ in snaps] + [host(envs.state64)])
    E = np.stack([host(e) for _, e in snaps] + [host(envs.elapsed)])
    acts = host(agent.b_act).T  # [T, n]
    assert acts.min() >= 0 and acts.max() <= 2
    r = ref.ref_step(ACROBOT, S[:-1].reshape(-1, 4), E[:-1].reshape(-1).astype(np.int64),
                     acts.reshape(-1), envs.max_episode_steps)
    ok = ~r['near']
    assert ok.mean() >= 0.99
    obs_buf = host(agent.obs_buf)  # [T + 1, n, 6]: the policy inputs, then the last obs
    assert np.abs(obs_buf[0].astype(np.float64) - ref.observe(ACROBOT, s_first)).max() <= 1e-6
    d_obs = np.abs(obs_buf[1:].reshape(-1, 6).astype(np.float64) - r['obs'])[ok].max()
    d_rew = np.abs(host(agent.b_rew).T.reshape(-1).astype(np.float64) - r['rew'])[ok].max()
    cont = ok & ~r['done']
    d_state = np.abs(S[1:].reshape(-1, 4) - r['state'])[cont].max()
    print(f'trpo acrobot: |obs| diff {d_obs:.3e}, |rew| diff {d_rew:.3e}, '
          f'|state| diff {d_state:.3e}')
    assert d_obs <= 1e-6 and d_rew <= 1e-6 and d_state <= 1e-9
    assert np.array_equal(host(agent.b_done)[:, 1:].T.reshape(-1)[ok] != 0, r['done'][ok])
    agent.train_step()  # the rollout is captured into a hipGraph and replayed from here on
    agent.train_step()
    for m in (actor, critic):
        assert np.isfinite(host(m.theta)).all()
    # the env went on stepping under the graph: 48 steps, its state still an Acrobot state
    fin = host(agent.b_done)[:, 1:].any()
    assert fin or (host(envs.elapsed) == 3 * T).all()
    s = host(envs.state64)
    assert np.abs(host(envs.state).astype(np.float64) - ref.observe(ACROBOT, s)).max() <= 1e-6
    assert (np.abs(s[:, :2]) <= np.pi).all() and not np.array_equal(s, S[-1])
