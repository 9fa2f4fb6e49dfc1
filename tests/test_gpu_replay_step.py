"""GPU test of xa_replay_env_step, the per-step kernel of every off-policy configuration,
called directly through the C ABI on a hand-made record.

The reference is a numpy restatement of BaseAgent.step_envs(store_in_buffers=True)
(xagents/base.py:388-426) over a recorded stream, with the two replay buffers of
xagents/utils/buffers.py (ReplayBuffer1: a deque of maxlen size; ReplayBuffer2: row
current_size % size, current_size saturating at size). It shares no code with the library.
Everything is compared with exact equality after every step: the kernels only move bytes and
do one f32 add per env (the episode return), which np.float32 addition reproduces.

Shapes (obs_bytes): 12 = one-launch kernel, byte moves; 96 = one-launch kernel, 16-byte moves;
4100 = frames + scalars kernels, byte moves, second 4096-byte chunk partial; 32784 = frames +
scalars kernels, 16-byte moves, last chunk partial. n_envs 65 crosses the 64-thread block of
the scalars kernel. t_rec 5, capacity 3 and 8 steps wrap the cursor and the ring.

Done pattern: env 0 never finishes an episode inside the 8 steps; every other env finishes at
least one (the test asserts both about its own inputs).
"""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

from xagents_amd import _lib

pytestmark = pytest.mark.gpu

T_REC, CAPACITY, STEPS = 5, 3, 8
OBS_BYTES = (12, 96, 4100, 32784)
N_ENVS = (3, 65)
ACT_BYTES = (4, 16)
RINGS = {'rb1': _lib.XA_RING_DEQUE, 'rb2': _lib.XA_RING_RB2, 'noring': None}
# (ring, out_states / out_new_states present, out_ld, done_epret present): every ring kind
# with and without the observation outputs, every out_ld and done_epret both ways with and
# without a ring
VARIANTS = (('rb1', True, 0, True), ('rb1', False, 4, False), ('rb2', True, 4, True),
            ('rb2', False, 1, False), ('noring', True, 1, True), ('noring', False, 0, False),
            ('rb2', True, 0, False), ('rb1', True, 1, True), ('noring', True, 4, False))
OBS_FILL, F32_FILL = 0xA5, -7.0  # what no step may leave behind where it does not write


@functools.lru_cache(maxsize=None)
def host_record(n, ob):
    """s0 [n, ob] u8, rep_obs / rep_state [n, T_REC, ob] u8, rep_rew / rep_done [n, T_REC]
    f32, the per-step actions [STEPS, n, 16] u8."""
    rng = np.random.default_rng(1000 * ob + n)
    s0 = rng.integers(0, 256, (n, ob), dtype=np.uint8)
    rep_obs = rng.integers(0, 256, (n, T_REC, ob), dtype=np.uint8)
    rep_state = rng.integers(0, 256, (n, T_REC, ob), dtype=np.uint8)
    rep_rew = rng.standard_normal((n, T_REC)).astype(np.float32)
    rep_done = (rng.random((n, T_REC)) < 0.4).astype(np.float32)
    rep_done[0] = 0.0                              # env 0 finishes no episode
    rep_done[np.arange(1, n), rng.integers(0, T_REC, n - 1)] = 1.0  # the others at least one
    actions = rng.integers(0, 256, (STEPS, n, max(ACT_BYTES)), dtype=np.uint8)
    return s0, rep_obs, rep_state, rep_rew, rep_done, actions


@functools.lru_cache(maxsize=None)
def device_record(n, ob):
    return tuple(torch.from_numpy(a).cuda() for a in host_record(n, ob))


class RB1:
    """ReplayBuffer1 (buffers.py:59-98): deque(maxlen=size). On the device the k-th append
    of an env lands on row k % size, so the rows in age order are the deque."""

    def __init__(self, size):
        self.size, self.count = size, 0
        self.main_buffer = collections.deque(maxlen=size)

    def append(self, *args):
        self.main_buffer.append(args)
        row = self.count % self.size
        self.count += 1
        return row


class RB2:
    """ReplayBuffer2 (buffers.py:101-148): row current_size % size, current_size saturating
    at size, so every append lands on row 0 once the buffer is full."""

    def __init__(self, size):
        self.size, self.count = size, 0

    def append(self, *args):
        row = self.count % self.size
        if self.count < self.size:
            self.count += 1
        return row


class Reference:
    """BaseAgent.step_envs over the recorded stream, env by env (base.py:402-425)."""

    def __init__(self, n, ob, act_bytes, ring):
        self.s0, self.rep_obs, self.rep_state, self.rep_rew, self.rep_done, _ = host_record(n, ob)
        self.n = n
        self.states = self.s0.copy()
        self.cursor = np.zeros(n, np.int32)
        self.dones = np.zeros(n, np.float32)
        self.episode_rewards = np.zeros(n, np.float32)
        self.buffers = None
        if ring is not None:
            self.buffers = [(RB2 if ring == _lib.XA_RING_RB2 else RB1)(CAPACITY)
                            for _ in range(n)]
            self.ring_states = np.full((n, CAPACITY, ob), OBS_FILL, np.uint8)
            self.ring_new_states = np.full((n, CAPACITY, ob), OBS_FILL, np.uint8)
            self.ring_actions = np.full((n, CAPACITY, act_bytes), OBS_FILL, np.uint8)
            self.ring_rewards = np.full((n, CAPACITY), F32_FILL, np.float32)
            self.ring_dones = np.full((n, CAPACITY), F32_FILL, np.float32)

    def step(self, actions):
        """Returns this step's (states, rewards, dones, new_states, finished-episode returns)."""
        obs = []
        for i in range(self.n):
            c = self.cursor[i]
            state = self.states[i].copy()
            # env.step: the recorded transition at the env's cursor
            new_state, reward, done = self.rep_obs[i, c], self.rep_rew[i, c], self.rep_done[i, c]
            self.cursor[i] = (c + 1) % T_REC
            self.states[i] = new_state
            self.dones[i] = done
            self.episode_rewards[i] = np.float32(self.episode_rewards[i] + reward)
            if self.buffers is not None:
                row = self.buffers[i].append(state, actions[i], reward, done, new_state)
                self.ring_states[i, row], self.ring_new_states[i, row] = state, new_state
                self.ring_actions[i, row] = actions[i]
                self.ring_rewards[i, row], self.ring_dones[i, row] = reward, done
            epret = np.float32(0.0)
            if done:
                epret = self.episode_rewards[i]
                self.episode_rewards[i] = 0
            # the state carried on is the record's post-step state: env.reset() where done;
            # the stream records one for every step, and the step stores it either way
            self.states[i] = self.rep_state[i, c]
            obs.append((state, reward, done, new_state.copy(), epret))
        return [np.array(x) for x in zip(*obs)]

    def ring_count(self):
        return np.array([b.count for b in self.buffers], np.int64)


def check_done_pattern(rep_done):
    episodes = rep_done[:, [t % T_REC for t in range(STEPS)]].sum(1)
    assert episodes[0] == 0 and (episodes[1:] >= 1).all()
    assert (episodes > 1).any()  # and somewhere the return restarts more than once


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: f'{v[0]}-outs{int(v[1])}-ld{v[2]}-'
                                                            f'epret{int(v[3])}')
@pytest.mark.parametrize('act_bytes', ACT_BYTES)
@pytest.mark.parametrize('n', N_ENVS)
@pytest.mark.parametrize('ob', OBS_BYTES)
def test_replay_env_step_matches_step_envs(device, ob, n, act_bytes, variant):
    ring_name, outs, out_ld, epret = variant
    ring = RINGS[ring_name]
    s0, rep_obs, rep_state, rep_rew, rep_done, actions = device_record(n, ob)
    actions = actions[:, :, :act_bytes].contiguous()
    acts_host = host_record(n, ob)[5][:, :, :act_bytes]
    ref = Reference(n, ob, act_bytes, ring)
    check_done_pattern(ref.rep_done)

    def full(shape, fill, dtype):
        return torch.full(shape, fill, dtype=dtype, device='cuda')

    u8, f32 = torch.uint8, torch.float32
    state = s0.clone()
    cursor = torch.zeros(n, dtype=torch.int32, device='cuda')
    done, ep_return = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    ld = max(out_ld, 1)
    out_rewards, out_dones = full((n, ld), F32_FILL, f32), full((n, ld), F32_FILL, f32)
    done_epret = full((n, ld), F32_FILL, f32)
    out_states, out_new_states = full((n, ob), OBS_FILL, u8), full((n, ob), OBS_FILL, u8)

    a = _lib.XaReplayStepArgs()
    a.n_envs, a.t_rec, a.obs_bytes = n, T_REC, ob
    a.rep_obs, a.rep_state = rep_obs.data_ptr(), rep_state.data_ptr()
    a.rep_rew, a.rep_done = rep_rew.data_ptr(), rep_done.data_ptr()
    a.state, a.cursor = state.data_ptr(), cursor.data_ptr()
    a.ep_return, a.done = ep_return.data_ptr(), done.data_ptr()
    a.out_rewards, a.out_dones, a.out_ld = out_rewards.data_ptr(), out_dones.data_ptr(), out_ld
    if epret:
        a.done_epret = done_epret.data_ptr()
    if outs:
        a.out_states, a.out_new_states = out_states.data_ptr(), out_new_states.data_ptr()
    if ring is not None:
        ring_states = full((n, CAPACITY, ob), OBS_FILL, u8)
        ring_new_states = full((n, CAPACITY, ob), OBS_FILL, u8)
        ring_actions = full((n, CAPACITY, act_bytes), OBS_FILL, u8)
        ring_rewards = full((n, CAPACITY), F32_FILL, f32)
        ring_dones = full((n, CAPACITY), F32_FILL, f32)
        ring_count = torch.zeros(n, dtype=torch.int64, device='cuda')
        a.capacity, a.ring_kind, a.ring_count = CAPACITY, ring, ring_count.data_ptr()
        a.ring_states, a.ring_new_states = ring_states.data_ptr(), ring_new_states.data_ptr()
        a.ring_actions, a.ring_rewards = ring_actions.data_ptr(), ring_rewards.data_ptr()
        a.ring_dones, a.act_bytes = ring_dones.data_ptr(), act_bytes

    for t in range(STEPS):
        for buf in (out_rewards, out_dones, done_epret):
            buf.fill_(F32_FILL)
        out_states.fill_(OBS_FILL)
        out_new_states.fill_(OBS_FILL)
        a.actions = actions[t].data_ptr() if ring is not None else None
        _lib.call('xa_replay_env_step', ctypes.byref(a), _lib.stream())
        torch.cuda.synchronize()
        r_states, r_rew, r_done, r_new, r_epret = ref.step(acts_host[t])

        def row0(x, filled):
            e = np.full((n, ld), F32_FILL, np.float32)
            if filled:
                e[:, 0] = x
            return e

        where = f'step {t}'
        assert np.array_equal(host(state), ref.states), where
        assert np.array_equal(host(cursor), ref.cursor), where
        assert np.array_equal(host(done), ref.dones), where
        assert np.array_equal(host(ep_return), ref.episode_rewards), where
        assert np.array_equal(host(out_rewards), row0(r_rew, True)), where
        assert np.array_equal(host(out_dones), row0(r_done, True)), where
        assert np.array_equal(host(done_epret), row0(r_epret, epret)), where
        exp_s = r_states if outs else np.full((n, ob), OBS_FILL, np.uint8)
        exp_n = r_new if outs else np.full((n, ob), OBS_FILL, np.uint8)
        assert np.array_equal(host(out_states), exp_s), where
        assert np.array_equal(host(out_new_states), exp_n), where
        if ring is not None:
            assert np.array_equal(host(ring_count), ref.ring_count()), where
            assert np.array_equal(host(ring_states), ref.ring_states), where
            assert np.array_equal(host(ring_new_states), ref.ring_new_states), where
            assert np.array_equal(host(ring_actions), ref.ring_actions), where
            assert np.array_equal(host(ring_rewards), ref.ring_rewards), where
            assert np.array_equal(host(ring_dones), ref.ring_dones), where

    if ring == _lib.XA_RING_DEQUE:
        # the rows in age order are ReplayBuffer1's deque
        for i, b in enumerate(ref.buffers):
            kept = len(b.main_buffer)
            rows = [(b.count - kept + k) % CAPACITY for k in range(kept)]
            for row, (s, act, rew, dn, ns) in zip(rows, b.main_buffer):
                assert np.array_equal(ref.ring_states[i, row], s)
                assert np.array_equal(ref.ring_new_states[i, row], ns)
                assert np.array_equal(ref.ring_actions[i, row], act)
                assert ref.ring_rewards[i, row] == rew and ref.ring_dones[i, row] == dn
    if ring == _lib.XA_RING_RB2:
        assert (ref.ring_count() == CAPACITY).all()  # saturated, not STEPS
