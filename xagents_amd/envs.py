"""Device-resident vectorized environments.

The reference steps a Python list of gym envs one by one (xagents/base.py:388-426,
created by create_envs, xagents/utils/common.py:145-166). Here the env state of
all n envs lives in HBM and is stepped inside the fused rollout kernel:

* ReplayVecEnv -- synthetic pre-recorded observation replay (BASELINE config 2):
  per env a recorded stream of (obs returned by step, post-reset state, reward,
  done) of length t_rec, generated once on the host from a CartPole-v1
  restatement with a seeded random policy; stepping advances a per-env cursor.
* CartPoleVecEnv -- gym CartPole-v1 dynamics (Euler, f64 state, TimeLimit 500)
  evaluated on device, actions applied.
* AcrobotVecEnv / MountainCarVecEnv -- gym Acrobot-v1 (book dynamics, RK4, TimeLimit 500)
  and MountainCar-v0 (TimeLimit 200) in the same fused rollout; ClassicControlVecEnv steps
  the same two dynamics one launch per env step (xa_classic_step) for the agents whose
  models run on the layer executor.
* ContinuousControlVecEnv -- gym Pendulum-v1 (TimeLimit 200) and MountainCarContinuous-v0
  (TimeLimit 999) for the continuous-action agents; the env step and the replay-ring append
  are one launch (xa_continuous_env_step).

All expose the gym-like surface the agents use: len(), observation_space.shape,
action_space (Discrete/Box), seed(), reset().
"""
import ctypes

import numpy as np
import torch

from xagents_amd._lib import (XA_ENV_ACROBOT, XA_ENV_CARTPOLE, XA_ENV_MOUNTAINCAR,
                              XA_ENV_MOUNTAINCAR_CONT, XA_ENV_PENDULUM, XA_ENV_REPLAY,
                              XaClassicStepArgs, XaContinuousStepArgs, XaWalkerStepArgs, call,
                              stream)
from xagents_amd.nets import default_device


class Discrete:
    def __init__(self, n):
        self.n = int(n)
        self.shape = ()
        self._rng = np.random.default_rng()

    def seed(self, seed):
        self._rng = np.random.default_rng(seed)

    def sample(self):
        return int(self._rng.integers(self.n))

    def __repr__(self):
        return f'Discrete({self.n})'


class Box:
    def __init__(self, low, high, shape, dtype=np.float32):
        self.low, self.high = low, high
        self.shape = tuple(shape)
        self.dtype = dtype
        self._rng = np.random.default_rng()

    def seed(self, seed):
        self._rng = np.random.default_rng(seed)

    def sample(self):
        return self._rng.uniform(self.low, self.high, self.shape).astype(self.dtype)

    def __repr__(self):
        return f'Box({self.low}, {self.high}, {self.shape}, {np.dtype(self.dtype).name})'


class EnvSpec:
    def __init__(self, id, max_episode_steps=None):
        self.id = id
        self.max_episode_steps = max_episode_steps


class CartPoleNumpy:
    """Vectorized CartPole-v1 restatement (gym classic_control/cartpole.py) in f64,
    used only to RECORD synthetic replay streams on the host."""

    gravity, masspole, total_mass, length = 9.8, 0.1, 1.1, 0.5
    polemass_length, force_mag, tau = 0.05, 10.0, 0.02
    theta_threshold = 12 * 2 * np.pi / 360
    x_threshold = 2.4

    def __init__(self, n, rng, max_episode_steps=500):
        self.n = n
        self.rng = rng
        self.max_episode_steps = max_episode_steps
        self.state = self.rng.uniform(-0.05, 0.05, (n, 4))
        self.elapsed = np.zeros(n, np.int64)

    def step(self, action):
        x, x_dot, theta, theta_dot = self.state.T
        force = np.where(action == 1, self.force_mag, -self.force_mag)
        costheta, sintheta = np.cos(theta), np.sin(theta)
        temp = (force + self.polemass_length * theta_dot ** 2 * sintheta) / self.total_mass
        thetaacc = (self.gravity * sintheta - costheta * temp) / (
            self.length * (4.0 / 3.0 - self.masspole * costheta ** 2 / self.total_mass))
        xacc = temp - self.polemass_length * thetaacc * costheta / self.total_mass
        x = x + self.tau * x_dot
        x_dot = x_dot + self.tau * xacc
        theta = theta + self.tau * theta_dot
        theta_dot = theta_dot + self.tau * thetaacc
        self.state = np.stack([x, x_dot, theta, theta_dot], 1)
        self.elapsed += 1
        done = ((x < -self.x_threshold) | (x > self.x_threshold)
                | (theta < -self.theta_threshold) | (theta > self.theta_threshold)
                | (self.elapsed >= self.max_episode_steps))
        obs = self.state.astype(np.float32)
        reset = self.rng.uniform(-0.05, 0.05, (self.n, 4))
        self.state = np.where(done[:, None], reset, self.state)
        self.elapsed = np.where(done, 0, self.elapsed)
        return obs, np.ones(self.n, np.float32), done, self.state.astype(np.float32)


def record_cartpole_replay(n_envs, t_rec, seed=55, max_episode_steps=500):
    """Record per-env CartPole-v1 streams under a uniform random policy
    (np.random.default_rng(seed)).

    Returns numpy arrays: s0 [N,4], rep_obs [N,t_rec,4] (obs returned by step p),
    rep_state [N,t_rec,4] (state after step p, post-reset), rep_rew [N,t_rec],
    rep_done [N,t_rec]. The last record of every env is forced terminal with
    post-state s0, so the cursor wrap-around is an ordinary episode boundary.
    """
    rng = np.random.default_rng(seed)
    env = CartPoleNumpy(n_envs, rng, max_episode_steps)
    s0 = env.state.astype(np.float32)
    rep_obs = np.empty((n_envs, t_rec, 4), np.float32)
    rep_state = np.empty((n_envs, t_rec, 4), np.float32)
    rep_rew = np.empty((n_envs, t_rec), np.float32)
    rep_done = np.empty((n_envs, t_rec), np.float32)
    for p in range(t_rec):
        obs, rew, done, post = env.step(rng.integers(0, 2, n_envs))
        rep_obs[:, p], rep_state[:, p], rep_rew[:, p] = obs, post, rew
        rep_done[:, p] = done
    rep_done[:, -1] = 1.0
    rep_state[:, -1] = s0
    return s0, rep_obs, rep_state, rep_rew, rep_done


class VecEnvBase:
    """The gym-like surface the agents use (len(), envs[0].observation_space, seed(), spec)
    and the reference's per-env BaseAgent.dones / episode_rewards (xagents/base.py:105-113)
    with the record cursor, kept in HBM."""

    def __init__(self, env_id, n_envs, observation_space, action_space, device=None):
        self.spec = EnvSpec(env_id)
        self.n_envs = int(n_envs)
        self.device = torch.device(device) if device is not None else default_device()
        self.observation_space = observation_space
        self.action_space = action_space
        n, dev = self.n_envs, self.device
        self.done = torch.zeros(n, dtype=torch.float32, device=dev)
        self.cursor = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ep_return = torch.zeros(n, dtype=torch.float32, device=dev)
        self._seed = None

    def __len__(self):
        return self.n_envs

    def __iter__(self):
        return iter([self] * self.n_envs)

    def __getitem__(self, i):
        return self  # envs[0].observation_space / action_space access pattern

    def seed(self, seed):
        self._seed = seed
        self.action_space.seed(seed)

    def _zero_episode_state(self):
        self.cursor.zero_()
        self.done.zero_()
        self.ep_return.zero_()


class DeviceVecEnv(VecEnvBase):
    """The envs of the fused rollout: the reference's BaseAgent.states (xagents/base.py:105-113)
    as an f32 row per env."""

    kind = None

    def __init__(self, env_id, n_envs, obs_shape, action_space, device=None):
        super().__init__(env_id, n_envs, Box(-np.inf, np.inf, obs_shape), action_space, device)
        self.obs_dim = int(np.prod(obs_shape))
        self.state = torch.zeros(self.n_envs, self.obs_dim, dtype=torch.float32,
                                 device=self.device)
        self.state64 = None

    def fill_rollout_args(self, a):
        a.env_kind = self.kind
        a.env_state = self.state.data_ptr()
        a.env_done = self.done.data_ptr()
        a.env_cursor = self.cursor.data_ptr()
        a.ep_return = self.ep_return.data_ptr()


class ReplayVecEnv(DeviceVecEnv):
    kind = XA_ENV_REPLAY

    def __init__(self, env_id='CartPole-v1', n_envs=1, t_rec=4096, seed=55, device=None,
                 record=None):
        super().__init__(env_id, n_envs, (4,), Discrete(2), device)
        s0, rep_obs, rep_state, rep_rew, rep_done = record or record_cartpole_replay(
            n_envs, t_rec, seed)
        self.t_rec = rep_obs.shape[1]
        dev = self.device
        self.s0 = torch.from_numpy(s0).to(dev)
        self.rep_obs = torch.from_numpy(np.ascontiguousarray(rep_obs)).to(dev)
        self.rep_state = torch.from_numpy(np.ascontiguousarray(rep_state)).to(dev)
        self.rep_rew = torch.from_numpy(np.ascontiguousarray(rep_rew)).to(dev)
        self.rep_done = torch.from_numpy(np.ascontiguousarray(rep_done)).to(dev)
        self.reset()

    def reset(self):
        self.state.copy_(self.s0)
        self._zero_episode_state()
        return self.state

    def fill_rollout_args(self, a):
        super().fill_rollout_args(a)
        a.rep_obs = self.rep_obs.data_ptr()
        a.rep_state = self.rep_state.data_ptr()
        a.rep_rew = self.rep_rew.data_ptr()
        a.rep_done = self.rep_done.data_ptr()
        a.t_rec = self.t_rec


def classic_initial_state(kind, n_envs, rng):
    """env.reset() of n_envs CartPole-v1 / Acrobot-v1 / MountainCar-v0 envs from a numpy
    generator: the f64 state [n, 4] (MountainCar: position, velocity = 0, two unused slots)
    and its f32 observation."""
    s = np.zeros((n_envs, 4))
    if kind == XA_ENV_CARTPOLE:
        s[:] = obs = rng.uniform(-0.05, 0.05, (n_envs, 4))
    elif kind == XA_ENV_ACROBOT:
        s[:] = rng.uniform(-0.1, 0.1, (n_envs, 4))
        obs = np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]),
                        s[:, 2], s[:, 3]], 1)
    else:
        s[:, 0] = rng.uniform(-0.6, -0.4, n_envs)
        obs = s[:, :2]
    return s, obs.astype(np.float32)


class ClassicDynamicsVecEnv(DeviceVecEnv):
    """CartPole-v1 / Acrobot-v1 / MountainCar-v0 dynamics in the fused rollout
    (csrc/classic_envs.hpp): f64 state [n, 4] on device, the policy sees its f32 observation."""

    env_id = None
    obs_dim_ = None
    n_actions = 3
    max_episode_steps = None

    def __init__(self, n_envs=1, seed=None, device=None):
        super().__init__(self.env_id, n_envs, (self.obs_dim_,), Discrete(self.n_actions), device)
        self.spec.max_episode_steps = self.max_episode_steps
        self.state64 = torch.zeros(self.n_envs, 4, dtype=torch.float64, device=self.device)
        self._seed = seed
        self.reset()

    def reset(self):
        s, obs = classic_initial_state(self.kind, self.n_envs, np.random.default_rng(self._seed))
        self.state64.copy_(torch.from_numpy(s))
        self.state.copy_(torch.from_numpy(obs))
        self._zero_episode_state()
        return self.state

    def fill_rollout_args(self, a):
        super().fill_rollout_args(a)
        a.env_state64 = self.state64.data_ptr()
        a.max_episode_steps = self.max_episode_steps


class CartPoleVecEnv(ClassicDynamicsVecEnv):
    kind = XA_ENV_CARTPOLE
    env_id, obs_dim_, n_actions, max_episode_steps = 'CartPole-v1', 4, 2, 500


class AcrobotVecEnv(ClassicDynamicsVecEnv):
    kind = XA_ENV_ACROBOT
    env_id, obs_dim_, max_episode_steps = 'Acrobot-v1', 6, 500


class MountainCarVecEnv(ClassicDynamicsVecEnv):
    kind = XA_ENV_MOUNTAINCAR
    env_id, obs_dim_, max_episode_steps = 'MountainCar-v0', 2, 200


CLASSIC_ENVS = {'Acrobot-v1': AcrobotVecEnv, 'MountainCar-v0': MountainCarVecEnv}


def record_transitions(n_envs, t_rec, obs_shape, dtype, seed=55, mean_episode=200,
                       reward_prob=0.02):
    """Synthetic pre-recorded transition streams for the off-policy configs
    (C3 Pong-shaped uint8 (84, 84, 1) frames i.i.d. uniform 0..255;
    C5 BipedalWalker-shaped f32 obs ~ N(0, 1)). Per env: s0, rep_obs [t_rec] (obs
    returned by step p), rep_state [t_rec] (post-reset state), rewards in {-1, 0, 1}
    (Pong-like, prob reward_prob each sign), episode ends ~ Geometric(1 / mean_episode);
    the last record is terminal with post-state s0 so the cursor wrap is an episode
    boundary. Generated from np.random.default_rng(seed)."""
    rng = np.random.default_rng(seed)
    shape = (n_envs, t_rec) + tuple(obs_shape)

    def frames(sh):
        if np.dtype(dtype) == np.uint8:
            return rng.integers(0, 256, size=sh, dtype=np.uint8)
        return rng.standard_normal(sh).astype(dtype)

    s0 = frames((n_envs,) + tuple(obs_shape))
    rep_obs = frames(shape)
    rep_done = (rng.random((n_envs, t_rec)) < 1.0 / mean_episode).astype(np.float32)
    rep_done[:, -1] = 1.0
    rep_state = rep_obs.copy()
    resets = frames(shape)
    m = rep_done.astype(bool)
    rep_state[m] = resets[m]
    rep_state[:, -1] = s0
    u = rng.random((n_envs, t_rec))
    rep_rew = np.where(u < reward_prob, 1.0, np.where(u > 1 - reward_prob, -1.0, 0.0))
    return s0, rep_obs, rep_state, rep_rew.astype(np.float32), rep_done


class TransitionReplayVecEnv(VecEnvBase):
    """Off-policy device env over pre-recorded transitions (Atari-shaped uint8 frames
    or continuous-control f32 vectors). Stepping -- and the replay-ring append of
    BaseAgent.step_envs(store_in_buffers=True), xagents/base.py:388-426 -- is one
    xa_replay_env_step launch; the actions are stored but do not change the stream."""

    def __init__(self, env_id, n_envs, obs_shape, action_space, obs_dtype=np.uint8,
                 t_rec=256, seed=55, device=None, record=None, mean_episode=200):
        self._setup(env_id, n_envs, obs_shape, action_space, obs_dtype, device)
        record = record or record_transitions(n_envs, t_rec, obs_shape, obs_dtype, seed,
                                              mean_episode)
        self._set_record(*(torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
                           for a in record))
        self.reset()

    def _setup(self, env_id, n_envs, obs_shape, action_space, obs_dtype, device):
        low, high = (0, 255) if np.dtype(obs_dtype) == np.uint8 else (-np.inf, np.inf)
        VecEnvBase.__init__(self, env_id, n_envs, Box(low, high, obs_shape, obs_dtype),
                            action_space, device)
        self.obs_dtype = np.dtype(obs_dtype)
        self.obs_shape = tuple(obs_shape)
        self.obs_bytes = int(np.prod(self.obs_shape)) * self.obs_dtype.itemsize

    def _set_record(self, s0, rep_obs, rep_state, rep_rew, rep_done):
        """The device record: s0 [N, *obs], rep_obs / rep_state [N, t_rec, *obs], rep_rew /
        rep_done [N, t_rec] f32."""
        self.t_rec = rep_obs.shape[1]
        self.s0, self.rep_obs, self.rep_state = s0, rep_obs, rep_state
        self.rep_rew, self.rep_done = rep_rew, rep_done
        self.state = torch.empty_like(s0)

    def reset(self):
        self.state.copy_(self.s0)
        self._zero_episode_state()
        return self.state

    def fill_step_args(self, a):
        a.n_envs, a.t_rec, a.obs_bytes = self.n_envs, self.t_rec, self.obs_bytes
        a.rep_obs, a.rep_state = self.rep_obs.data_ptr(), self.rep_state.data_ptr()
        a.rep_rew, a.rep_done = self.rep_rew.data_ptr(), self.rep_done.data_ptr()
        a.state, a.cursor = self.state.data_ptr(), self.cursor.data_ptr()
        a.ep_return, a.done = self.ep_return.data_ptr(), self.done.data_ptr()

    @property
    def has_pre_step(self):
        """Whether a launch of the env's own (pre_step) precedes every xa_replay_env_step."""
        return getattr(self, 'pre_step', None) is not None

    def step_into(self, args, actions=None, act_ld=None):
        """One env step into `args` (XaReplayStepArgs from fill_step_args, outputs pointed
        where the caller wants them): the env's pre_step, if it has one, with the step's
        actions (a device tensor, or a pointer and its stride act_ld), then
        xa_replay_env_step."""
        pre_step = getattr(self, 'pre_step', None)  # looked up per call: it may be wrapped
        if pre_step is not None:
            # raw-frame env (AtariWrapper.step) / dynamics env (env.step with the actions)
            # into the one-step record
            if act_ld is None:
                pre_step(actions)
            else:
                pre_step(actions, act_ld)
        call('xa_replay_env_step', ctypes.byref(args), stream())


class StepKernelVecEnv(TransitionReplayVecEnv):
    """Base of the envs a kernel of their own steps (pre_step) into a one-step record
    (t_rec == 1), which xa_replay_env_step then consumes like a recorded transition.
    Subclasses allocate their state and end their constructor with self.reset()."""

    def __init__(self, env_id, n_envs, obs_shape, action_space, obs_dtype, device=None):
        self._setup(env_id, n_envs, obs_shape, action_space, obs_dtype, device)
        n, shape = self.n_envs, self.obs_shape
        dtype = torch.uint8 if self.obs_dtype == np.uint8 else torch.float32
        obs = dict(dtype=dtype, device=self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._set_record(torch.zeros((n,) + shape, **obs), torch.zeros((n, 1) + shape, **obs),
                         torch.zeros((n, 1) + shape, **obs), torch.zeros(n, 1, **f32),
                         torch.zeros(n, 1, **f32))

    def record_ptrs(self):
        """(obs, post-reset state, reward, done) of the one-step record."""
        return (self.rep_obs.data_ptr(), self.rep_state.data_ptr(), self.rep_rew.data_ptr(),
                self.rep_done.data_ptr())


class DynamicsStepVecEnv(StepKernelVecEnv):
    """Base of the envs whose dynamics a step kernel of their own evaluates with the step's
    actions: the entry point, its argument struct and the action layout (act_width elements of
    act_dtype per env) are class attributes, _fill_args points the struct at the env's own
    memory. Resets draw from Philox keyed by the env's seed and a device counter that only
    steps or finished episodes advance."""

    entry = args_type = act_dtype = act_width = None

    def __init__(self, env_id, n_envs, obs_shape, action_space, seed, device):
        super().__init__(env_id, n_envs, obs_shape, action_space, np.float32, device)
        self.env_seed = int(seed if seed is not None else 0) % 2**64

    def _args(self, reset_only, actions=0, act_ld=None):
        a = self.args_type()
        a.n_envs, a.seed, a.reset_only = self.n_envs, self.env_seed, int(reset_only)
        a.actions, a.act_ld = actions, self.act_width if act_ld is None else act_ld
        self._fill_args(a)
        return a

    def _launch(self, a):
        call(self.entry, ctypes.byref(a), stream())

    def reset(self):
        """env.reset() of every env into the state. The draw's counter does not move without
        steps, so repeated reset() calls without steps in between replay the same initial
        state."""
        super().reset()
        a = self._args(True)
        a.out_post = self.state.data_ptr()
        self._launch(a)
        return self.state

    def _action_ptr(self, actions, act_ld=None):
        """(pointer, stride in elements between envs) of the step's actions: a contiguous
        device tensor of n_envs x act_width act_dtype elements, or a raw pointer and its
        act_ld."""
        if actions is None:
            raise ValueError(f'{type(self).__name__} needs the step\'s actions')
        if isinstance(actions, int):
            return actions, self.act_width if act_ld is None else act_ld
        assert actions.dtype == self.act_dtype and actions.is_contiguous() and \
            actions.numel() == self.n_envs * self.act_width
        return actions.data_ptr(), self.act_width

    def record_step(self, actions=None, act_ld=None):
        """env.step of every env with `actions` into the one-step record (the pre_step of the
        two-launch step)."""
        a = self._args(False, *self._action_ptr(actions, act_ld))
        a.out_obs, a.out_post, a.out_rew, a.out_done = self.record_ptrs()
        self._launch(a)


class WalkerVecEnv(DynamicsStepVecEnv):
    """BipedalWalker-v3 device stand-in (csrc/walker.hip): real
    action-dependent dynamics with BipedalWalker's 24-value observation, 4 motor commands
    in [-1, 1], reward formula and termination (not Box2D: a planar kinematic walker on flat
    ground). Each env step is one xa_walker_step launch (pre_step, given the step's actions)
    into the one-step record that xa_replay_env_step then turns into the agent's state,
    rewards, dones and replay-ring append, as for the other transition envs. The initial push
    is drawn from the env's episode counter, which only a finished episode advances."""

    entry, args_type, act_dtype, act_width = 'xa_walker_step', XaWalkerStepArgs, torch.float32, 4
    pre_step = DynamicsStepVecEnv.record_step

    def __init__(self, env_id='BipedalWalker-v3', n_envs=1, seed=55, device=None):
        super().__init__(env_id, n_envs, (24,), Box(-1.0, 1.0, (4,)), seed, device)
        self.walker_seed = self.env_seed
        self.walker_state = torch.zeros(self.n_envs, 18, dtype=torch.float32, device=self.device)
        self.episode = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        self.reset()

    def _fill_args(self, a):
        a.state, a.episode = self.walker_state.data_ptr(), self.episode.data_ptr()


class ClassicControlVecEnv(DynamicsStepVecEnv):
    """Acrobot-v1 / MountainCar-v0 behind the executor env step (csrc/classic_envs.hip): the
    dynamics of AcrobotVecEnv / MountainCarVecEnv, bit for bit, one xa_classic_step launch
    per env step (pre_step, given the step's actions) into the one-step record that
    xa_replay_env_step then turns into the agent's state, rewards, dones and replay-ring
    append, as for the other transition envs. Resets draw from Philox keyed by the env's
    seed and its own device step counter."""

    entry, args_type, act_dtype, act_width = 'xa_classic_step', XaClassicStepArgs, torch.int32, 1

    def __init__(self, env_id='Acrobot-v1', n_envs=1, seed=55, device=None):
        fused = CLASSIC_ENVS[env_id]
        super().__init__(env_id, n_envs, (fused.obs_dim_,), Discrete(3), seed, device)
        self.kind = fused.kind
        self.max_episode_steps = fused.max_episode_steps
        self.spec.max_episode_steps = self.max_episode_steps
        self.state64 = torch.zeros(self.n_envs, 4, dtype=torch.float64, device=self.device)
        self.elapsed = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        # position of the reset-draw stream: one per env step, read on device (so a
        # captured rollout draws fresh resets on every replay)
        self.step_counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        # pre_step(tensor) validates the actions on the host (one sync per step); raw
        # pointers (the on-policy rollouts, whose sampler cannot leave [0, 3)) are not
        self.check_actions = True
        self.reset()

    def _fill_args(self, a):
        a.env_kind, a.max_episode_steps = self.kind, self.max_episode_steps
        a.state64, a.elapsed = self.state64.data_ptr(), self.elapsed.data_ptr()
        # step index of the launch's reset draws; -1 for reset(): no step's draw uses it
        a.counter, a.t = self.step_counter.data_ptr(), -1 if a.reset_only else 0

    def pre_step(self, actions=None, act_ld=None):
        """env.step of every env with `actions` (a device tensor [N] int32, or a pointer to
        int32 actions at element stride act_ld) into the one-step record."""
        if not isinstance(actions, int) and actions is not None and self.check_actions and \
                not torch.cuda.is_current_stream_capturing():
            lo, hi = int(actions.min()), int(actions.max())
            if lo < 0 or hi >= self.action_space.n:
                raise ValueError(f'actions must lie in [0, {self.action_space.n}), got '
                                 f'[{lo}, {hi}]')
        self.record_step(actions, act_ld)
        call('xa_counter_bump', self.step_counter.data_ptr(), stream())


# id -> (env kind, observation size, action bound, gym's TimeLimit)
CONTINUOUS_ENVS = {'Pendulum-v1': (XA_ENV_PENDULUM, 3, 2.0, 200),
                   'MountainCarContinuous-v0': (XA_ENV_MOUNTAINCAR_CONT, 2, 1.0, 999)}


class ContinuousControlVecEnv(DynamicsStepVecEnv):
    """Pendulum-v1 / MountainCarContinuous-v0 on device (csrc/continuous_envs.hip): f64 state
    [n, 2], one f32 action per env, clipped by the env as gym does. step_into is ONE
    xa_continuous_env_step launch doing env.step / env.reset and what xa_replay_env_step does
    with the result (agent state, rewards, dones, replay-ring append), so the env has no
    pre_step and the off-policy agents keep it on their staged env phase. fused=False is the
    two-launch composition the other step-kernel envs use (record_step as pre_step, then
    xa_replay_env_step), kept for A/B timing and the equality tests: same bits. Resets draw
    from Philox keyed by the env's seed, its index and its own episode counter.
    max_episode_steps=None takes the id's TimeLimit."""

    entry, args_type = 'xa_continuous_env_step', XaContinuousStepArgs
    act_dtype, act_width = torch.float32, 1

    def __init__(self, env_id='Pendulum-v1', n_envs=1, seed=55, device=None,
                 max_episode_steps=None, fused=True):
        kind, obs_dim, bound, limit = CONTINUOUS_ENVS[env_id]
        limit = int(limit if max_episode_steps is None else max_episode_steps)
        if limit <= 0:
            raise ValueError(f'max_episode_steps must be > 0, got {max_episode_steps}')
        super().__init__(env_id, n_envs, (obs_dim,), Box(-bound, bound, (1,)), seed, device)
        self.kind = kind
        self.max_episode_steps = limit
        self.spec.max_episode_steps = limit
        self.state64 = torch.zeros(self.n_envs, 2, dtype=torch.float64, device=self.device)
        self.elapsed = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        self.episode = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        self.fused = bool(fused)
        if not self.fused:
            self.pre_step = self.record_step
        self._step_a = self._args(False)  # the launch arguments of a step, built once
        self.reset()

    def _fill_args(self, a):
        a.env_kind, a.max_episode_steps = self.kind, self.max_episode_steps
        a.state64, a.elapsed = self.state64.data_ptr(), self.elapsed.data_ptr()
        a.episode = self.episode.data_ptr()

    def _launch(self, a, step=None):
        call(self.entry, ctypes.byref(a), None if step is None else ctypes.byref(step), stream())

    def _step_args_for(self, actions, act_ld):
        a = self._step_a
        a.actions, a.act_ld = self._action_ptr(actions, act_ld)
        return a

    def step_into(self, args, actions=None, act_ld=None):
        """One env step into `args` (XaReplayStepArgs from fill_step_args, outputs pointed
        where the caller wants them) in one launch; the two-launch form when the instance
        has a pre_step (fused=False, or a wrapper someone installed)."""
        if getattr(self, 'pre_step', None) is not None:
            return super().step_into(args, actions, act_ld)
        self._launch(self._step_args_for(actions, act_ld), args)


def create_envs(env_name, n=1, preprocess=False, *args, mode=None, seed=55, device=None,
                t_rec=4096, **kwargs):
    """Device counterpart of xagents.utils.common.create_envs (common.py:145-166).

    Returns ONE vectorized env object of length n (the agents accept it wherever the
    reference takes a list of gym envs). mode: 'replay' (recorded streams; the default for
    every id that has them), 'dynamics' (the env stepped on device with the actions; the
    default for Acrobot-v1 and MountainCar-v0, which have no recorded mode) or
    'transitions' (the transition-replay surface the layer-executor agents step).
    Pendulum-v1 and MountainCarContinuous-v0 are one env (ContinuousControlVecEnv, which
    takes max_episode_steps / fused from kwargs) under 'dynamics' and 'transitions' alike.
    """
    if env_name in CLASSIC_ENVS:
        assert not preprocess, (f'Cannot use AtariWrapper or --preprocess for non-atari '
                                f'environment {env_name}')
        if mode is None or mode == 'dynamics':
            return CLASSIC_ENVS[env_name](n, seed=seed, device=device)
        if mode == 'transitions':
            return ClassicControlVecEnv(env_name, n, seed=seed, device=device)
        raise ValueError(f"{env_name} has no mode {mode!r}: use 'dynamics' (fused rollout) "
                         f"or 'transitions' (step kernel)")
    if env_name in CONTINUOUS_ENVS:
        assert not preprocess, (f'Cannot use AtariWrapper or --preprocess for non-atari '
                                f'environment {env_name}')
        if mode not in (None, 'dynamics', 'transitions'):
            raise ValueError(f"{env_name} has no mode {mode!r}: use 'dynamics' or "
                             f"'transitions' (the same step-kernel env)")
        return ContinuousControlVecEnv(env_name, n, seed=seed, device=device, **kwargs)
    if mode is None:
        mode = 'replay'
    if 'NoFrameskip' in env_name and preprocess:
        # AtariWrapper on device over a synthetic raw RGB frame stream (atari.py)
        from xagents_amd.atari import AtariFrameVecEnv
        actions = {'PongNoFrameskip-v4': 6, 'BreakoutNoFrameskip-v4': 4}.get(env_name, 6)
        return AtariFrameVecEnv(env_name, n, actions, *args, seed=seed, device=device,
                                t_raw=kwargs.pop('t_raw_frames', 64), **kwargs)
    if 'NoFrameskip' in env_name:
        # Atari-shaped synthetic replay: frames as AtariWrapper emits them (84, 84, 1)
        # uint8 (xagents/utils/common.py:67-142); the wrapper itself is not rebuilt
        actions = {'PongNoFrameskip-v4': 6, 'BreakoutNoFrameskip-v4': 4}.get(env_name, 6)
        return TransitionReplayVecEnv(env_name, n, (84, 84, 1), Discrete(actions), np.uint8,
                                      t_rec=min(t_rec, 256), seed=seed, device=device)
    if env_name.startswith('BipedalWalker'):
        if mode == 'dynamics':
            return WalkerVecEnv(env_name, n, seed=seed, device=device)
        return TransitionReplayVecEnv(env_name, n, (24,), Box(-1.0, 1.0, (4,)), np.float32,
                                      t_rec=t_rec, seed=seed, device=device)
    assert not preprocess, (f'Cannot use AtariWrapper or --preprocess for non-atari '
                            f'environment {env_name}')
    if env_name != 'CartPole-v1':
        raise NotImplementedError(f'No device environment for {env_name}')
    if mode == 'replay':
        return ReplayVecEnv(env_name, n, t_rec=t_rec, seed=seed, device=device)
    if mode == 'dynamics':
        return CartPoleVecEnv(n, seed=seed, device=device)
    if mode == 'transitions':
        # the same CartPole record behind the executor env step (models run by the layer
        # executor, e.g. TRPO's separate actor and critic)
        return TransitionReplayVecEnv(env_name, n, (4,), Discrete(2), np.float32, seed=seed,
                                      device=device,
                                      record=record_cartpole_replay(n, t_rec, seed))
    raise ValueError(f'Unknown env mode {mode}')
