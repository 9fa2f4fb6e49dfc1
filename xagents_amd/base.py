"""BaseAgent / OnPolicy / OffPolicy with the reference's class surface
(xagents/base.py:22-751). The host-side bookkeeping (metrics, checkpoints, early
stopping, history) is kept in Python as in the reference; env stepping, batching
and math go to libxagents_hip.so through the subclasses.

Differences forced by the device design (documented in DESIGN.md):
* `envs` is a device vector env (xagents_amd.envs) rather than a list of gym envs;
  it supports len(), envs[0].observation_space / action_space.
* Episode statistics reach total_rewards / games / done_envs asynchronously, one train_step
  late, in the reference's step-major, env-minor order (xagents_amd/episode_stats.py).
"""
import os
import random
from abc import ABC
from collections import deque
from datetime import timedelta
from pathlib import Path
from time import perf_counter

import numpy as np
import torch
import torch.distributed as dist

from xagents_amd.envs import Box, Discrete
from xagents_amd.utils.common import write_from_dict


class BaseAgent(ABC):
    def __init__(
        self,
        envs,
        model,
        checkpoints=None,
        reward_buffer_size=100,
        n_steps=1,
        gamma=0.99,
        display_precision=2,
        seed=None,
        log_frequency=None,
        history_checkpoint=None,
        plateau_reduce_factor=0.9,
        plateau_reduce_patience=10,
        early_stop_patience=3,
        divergence_monitoring_steps=None,
        quiet=False,
        trial=None,
    ):
        assert envs, 'No environments given'
        self.n_envs = len(envs)
        self.envs = envs
        self.model = model
        self.checkpoints = checkpoints
        self.total_rewards = deque(maxlen=reward_buffer_size)
        self.n_steps = n_steps
        self.gamma = gamma
        self.display_precision = display_precision
        self.seed = seed
        self.output_models = [self.model]
        self.log_frequency = log_frequency or self.n_envs
        # the agent package (xagents/base.py:88); a user subclass defined outside the
        # package (the reference would fail here) takes its nearest agent base class's id
        self.id = next((c.__module__.split('.')[1] for c in type(self).__mro__
                        if c.__module__.startswith('xagents_amd.')), self.__module__)
        self.history_checkpoint = history_checkpoint
        self.plateau_reduce_factor = plateau_reduce_factor
        self.plateau_reduce_patience = plateau_reduce_patience
        self.early_stop_patience = early_stop_patience
        self.divergence_monitoring_steps = divergence_monitoring_steps
        self.quiet = quiet
        self.trial = trial
        self.reported_rewards = 0
        self.plateau_count = 0
        self.early_stop_count = 0
        self.target_reward = None
        self.max_steps = None
        self.input_shape = self.envs[0].observation_space.shape
        self.n_actions = None
        self.best_reward = -float('inf')
        self.mean_reward = -float('inf')
        self.device = getattr(envs, 'device', torch.device('cuda'))
        self.dones = [False] * self.n_envs
        self.steps = 0
        self.frame_speed = 0
        self.last_reset_step = 0
        self.training_start_time = None
        self.last_reset_time = None
        self.games = 0
        self.episode_rewards = np.zeros(self.n_envs)
        self.done_envs = 0
        self.supported_action_spaces = Box, Discrete
        self.episode_stats = None  # on-policy rollouts: EpisodeStats, built with the buffers
        self.device_status = None  # a persistent update's status word (PPO)
        if seed:
            self.set_seeds(seed)
        self.reset_envs()
        self.set_action_count()
        self.img_inputs = len(self.input_shape) >= 2
        self.display_titles = (
            'time',
            'steps',
            'games',
            'speed',
            'mean reward',
            'best reward',
        )

    # ---- reference surface (host bookkeeping) -----------------------------
    def assert_valid_env(self, env, valid_type):
        assert isinstance(env.action_space, valid_type), (
            f'Invalid environment: {env.spec.id}. {self.__class__.__name__} supports '
            f'environments with a {valid_type} action space only, got {env.action_space}'
        )

    def display_message(self, *args, **kwargs):
        if not self.quiet:
            print(*args, **kwargs)

    def set_seeds(self, seed):
        torch.manual_seed(seed)
        np.random.seed(seed)
        self.envs.seed(seed)
        os.environ['PYTHONHASHSEED'] = f'{seed}'
        random.seed(seed)

    def reset_envs(self):
        self.envs.reset()

    @property
    def states(self):
        """Per-env view of the current (post-reset) observations, as the reference's list
        (LazyFrames for Atari frames, xagents/base.py:105-113); the device path reads
        self.envs.state directly."""
        from xagents_amd.utils.common import DeviceStates
        return DeviceStates(self.envs.state)

    def set_action_count(self):
        action_space = self.envs[0].action_space
        assert (
            type(action_space) in self.supported_action_spaces
        ), f'Expected one of {self.supported_action_spaces}, got {action_space}'
        if isinstance(action_space, Discrete):
            self.n_actions = action_space.n
        if isinstance(action_space, Box):
            self.n_actions = action_space.shape[0]

    def check_checkpoints(self):
        n_models = len(self.output_models)
        n_checkpoints = len(self.checkpoints)
        assert n_models == n_checkpoints, (
            f'Expected {n_models} checkpoints for {n_models} '
            f'given output models, got {n_checkpoints}'
        )

    def checkpoint(self):
        if self.mean_reward > self.best_reward:
            self.plateau_count = 0
            self.early_stop_count = 0
            self.display_message(
                f'Best reward updated: {self.best_reward} -> {self.mean_reward}'
            )
            if self.checkpoints:
                # a persistent launch that failed (device status word) left the weights
                # invalid: raise before any of them reaches a checkpoint file
                checks = getattr(self, '_device_checks', None)
                if checks is not None:
                    checks()
                for model, checkpoint in zip(self.output_models, self.checkpoints):
                    model.save_weights(checkpoint)
        self.best_reward = max(self.mean_reward, self.best_reward)

    def display_metrics(self):
        display_values = (
            timedelta(seconds=perf_counter() - self.training_start_time),
            self.steps,
            self.games,
            f'{round(self.frame_speed)} steps/s',
            self.mean_reward,
            self.best_reward,
        )
        display = (
            f'{title}: {value}'
            for title, value in zip(self.display_titles, display_values)
        )
        self.display_message(', '.join(display))

    def update_metrics(self):
        self.checkpoint()
        if (
            self.divergence_monitoring_steps
            and self.steps >= self.divergence_monitoring_steps
            and self.mean_reward <= self.best_reward
        ):
            self.plateau_count += 1
        if self.plateau_count >= self.plateau_reduce_patience:
            current_lr, new_lr = None, None
            pending = getattr(self, '_pending_lr', None)
            for model in self.output_models:
                current_lr = model.optimizer.learning_rate
                if pending is not None and model is self.output_models[-1]:
                    # data parallel: a reduction not applied yet (it waits for the next
                    # _dp_sync) compounds with this one, as the reference's would
                    current_lr = pending
                new_lr = current_lr * self.plateau_reduce_factor
            self.display_message(f'Learning rate reduced {current_lr} -> {new_lr}')
            if getattr(self, 'distributed', False):
                # data parallel: rank 0 decides, every rank applies it at the same train
                # step (_dp_sync), so learning rates and launch state stay identical
                if self.rank == 0:
                    self._pending_lr = new_lr
            else:
                # the reference only updates the LAST output model (xagents/base.py:277-284)
                self.output_models[-1].optimizer.learning_rate = new_lr
                self._on_lr_change()
            self.plateau_count = 0
            self.early_stop_count += 1
        self.frame_speed = (self.steps - self.last_reset_step) / (
            perf_counter() - self.last_reset_time
        )
        self.last_reset_step = self.steps
        self.mean_reward = np.around(
            np.mean(self.total_rewards), self.display_precision
        )

    def _on_lr_change(self):
        """Subclasses holding captured graphs re-capture them (lr is a kernel arg)."""

    # data parallel: the host decisions that must agree across ranks -- plateau learning-
    # rate reductions and stopping on the target reward / early-stop patience, which the
    # reference's one process takes from its own rewards -- are rank 0's, exchanged every
    # DP_SYNC_STEPS train steps of fit() and applied by every rank at the same step
    DP_SYNC_STEPS = 64

    def _dp_sync(self, stop_local):
        """One small collective (MAX over ranks): rank 0's pending learning rate and stop
        decision. Returns the agreed stop decision."""
        lr0 = getattr(self, '_pending_lr', None)
        t = torch.tensor([lr0 if (self.rank == 0 and lr0 is not None) else -1.0,
                          1.0 if (self.rank == 0 and stop_local) else 0.0], dtype=torch.float64)
        if dist.get_backend() != 'gloo':
            t = t.to(self.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        lr, stop = float(t[0].item()), bool(t[1].item() > 0)
        self._pending_lr = None
        if lr > 0:
            self.output_models[-1].optimizer.learning_rate = lr
            self._on_lr_change()
        return stop

    def _fit_done(self):
        """training_done(), collective in data-parallel runs: max_steps is identical on every
        rank (equal step counts); the reward-based decisions are rank 0's (_dp_sync)."""
        done = self.training_done()
        if not getattr(self, 'distributed', False):
            return done
        if self.max_steps and self.steps >= self.max_steps:
            return True
        self._fit_steps = getattr(self, '_fit_steps', 0) + 1
        every = int(os.environ.get('XA_DP_SYNC_STEPS', self.DP_SYNC_STEPS))
        if self._fit_steps % every:
            return False
        return self._dp_sync(done)

    def report_rewards(self):
        self.trial.report(np.mean(self.total_rewards), self.reported_rewards)
        self.reported_rewards += 1
        if self.trial.should_prune():
            import optuna

            raise optuna.exceptions.TrialPruned()

    def check_episodes(self):
        self._drain_episode_stats()
        if self.done_envs >= self.log_frequency:
            self.update_metrics()
            if self.trial:
                self.report_rewards()
            self.last_reset_time = perf_counter()
            self.display_metrics()
            self.done_envs = 0

    def training_done(self):
        if self.early_stop_count >= self.early_stop_patience:
            self.display_message('Early stopping')
            return True
        if self.target_reward and self.mean_reward >= self.target_reward:
            self.display_message(f'Reward achieved in {self.steps} steps')
            return True
        if self.max_steps and self.steps >= self.max_steps:
            self.display_message('Maximum steps exceeded')
            return True
        return False

    def concat_buffer_samples(self):
        """Concatenate per-env buffer samples (xagents/base.py:344-368)."""
        if hasattr(self, 'buffers'):
            batches = []
            for i in range(self.n_envs):
                batches.append(self.buffers[i].get_sample())
            dtypes = (
                self.batch_dtypes
                if hasattr(self, 'batch_dtypes')
                else [np.float32 for _ in range(len(batches[0]))]
            )
            if len(batches) > 1:
                return [
                    np.concatenate(item).astype(dtype)
                    for (item, dtype) in zip(zip(*batches), dtypes)
                ]
            return [item.astype(dtype) for (item, dtype) in zip(batches[0], dtypes)]

    def update_history(self, episode_reward):
        data = {
            'mean_reward': [self.mean_reward],
            'best_reward': [self.best_reward],
            'episode_reward': [episode_reward],
            'step': [self.steps],
            'time': [perf_counter() - self.training_start_time],
        }
        write_from_dict(data, self.history_checkpoint)

    def init_from_checkpoint(self):
        import pandas as pd

        previous_history = pd.read_parquet(self.history_checkpoint)
        expected_columns = {'time', 'mean_reward', 'best_reward', 'step', 'episode_reward'}
        assert (
            set(previous_history.columns) == expected_columns
        ), f'Expected the following columns: {expected_columns}, got {set(previous_history.columns)}'
        last_row = previous_history.loc[previous_history['time'].idxmax()]
        self.mean_reward = last_row['mean_reward']
        self.best_reward = previous_history['best_reward'].max()
        history_start_steps = last_row['step']
        history_start_time = last_row['time']
        self.training_start_time = perf_counter() - history_start_time
        self.last_reset_step = self.steps = int(history_start_steps)
        self.total_rewards.append(last_row['episode_reward'])
        self.games = previous_history.shape[0]

    def init_training(self, target_reward, max_steps, monitor_session):
        self.target_reward = target_reward
        self.max_steps = max_steps
        if monitor_session:
            import wandb

            wandb.init(name=monitor_session)
        if self.checkpoints:
            self.check_checkpoints()
        self.training_start_time = perf_counter()
        self.last_reset_time = perf_counter()
        if self.history_checkpoint and Path(self.history_checkpoint).exists():
            self.init_from_checkpoint()

    def train_step(self):
        raise NotImplementedError(
            f'train_step() should be implemented by {self.__class__.__name__} subclasses'
        )

    def get_model_outputs(self, inputs, models, training=True):
        if self.img_inputs:
            inputs = torch.as_tensor(inputs, device=self.device).float() / 255.0
        if not isinstance(models, (list, tuple)):
            return models(inputs, training=training)
        elif len(models) == 1:
            return models[0](inputs, training=training)
        return [sub_model(inputs, training=training) for sub_model in models]

    def at_step_start(self):
        pass

    def at_step_end(self):
        pass

    def get_states(self):
        """Most recent (post-reset) states, [n_envs, *obs] on device."""
        return self.envs.state

    def get_dones(self):
        return self.envs.done

    @staticmethod
    def concat_step_batches(*args):
        """Time-major [T, N, ...] -> env-major flat [N*T, ...] (xagents/base.py:549-564).

        Works on numpy arrays and torch tensors. The device rollout already stores its
        buffers env-major, so the fused path never needs this copy."""
        concatenated = []
        for arg in args:
            if len(arg.shape) == 1:
                arg = arg[..., None] if isinstance(arg, torch.Tensor) else np.expand_dims(arg, -1)
            if isinstance(arg, torch.Tensor):
                concatenated.append(arg.transpose(0, 1).reshape(-1, *arg.shape[2:]))
            else:
                concatenated.append(arg.swapaxes(0, 1).reshape(-1, *arg.shape[2:]))
        return concatenated

    # ---- device episode bookkeeping (xagents_amd/episode_stats.py) ------------
    # steps folded behind one event: half the in-launch statistics slots (_lib.XA_PPO_STATS_SLOTS)
    FUSED_GROUP_MAX = 8

    def _record_finished(self, finished):
        """Finished episodes' returns, in step_envs order (one extend: ~1,300 per C2 step)."""
        if not len(finished):
            return
        if self.history_checkpoint:
            for ret in finished:
                self.update_history(ret)
        self.total_rewards.extend(finished.astype(np.float64).tolist())
        self.games += len(finished)
        self.done_envs += len(finished)

    _stats_fused = property(lambda self: self.episode_stats is not None and
                            self.episode_stats.fused_on)

    def _queue_episode_stats(self, after=None, group_end=True):
        self.episode_stats.queue(after, group_end)

    def _sync_stats_copy(self):
        self.episode_stats.sync_copy()

    def _drain_episode_stats(self):
        if self.episode_stats is not None:
            self.episode_stats.drain()

    def fit(
        self,
        target_reward=None,
        max_steps=None,
        monitor_session=None,
    ):
        assert (
            target_reward or max_steps
        ), '`target_reward` or `max_steps` should be specified when fit() is called'
        self.init_training(target_reward, max_steps, monitor_session)
        while True:
            self.check_episodes()
            if self._fit_done():
                break
            self.at_step_start()
            self.train_step()
            self.at_step_end()
        self._drain_episode_stats()

    def play(self, video_dir=None, render=False, frame_dir=None, frame_delay=0.0,
             max_steps=None, action_idx=0, frame_frequency=1):
        """Play one game of env 0 with the current policy (xagents/base.py:595-653): reset
        the envs, act with the agent's play policy (A2C / PPO: a Categorical sample of the
        actor, DQN: argmax Q, DDPG / TD3: the noise-free actor), stop at env 0's first done
        or after max_steps steps, display the total reward.

        The envs are device envs, stepped together in chunks (_play_chunk); env 0's
        rewards and dones are read back per chunk and the reference's per-step loop runs
        over them. Nothing is rendered: video_dir / render / frame_dir need gym's renderer
        and cv2, which this build has no counterpart of. Training counters (steps, games,
        total_rewards) are left untouched, as the reference's play leaves them. Returns the
        total reward (the reference returns None)."""
        if video_dir or render or frame_dir:
            raise NotImplementedError(
                'play(): device envs have no renderer (video_dir / render / frame_dir need '
                'gym and cv2)')
        del frame_delay, action_idx, frame_frequency  # rendering / multi-output options
        self.reset_envs()
        total_reward, steps = 0.0, 0
        while True:
            rewards, dones = self._play_chunk()
            for r, d in zip(rewards, dones):
                if max_steps and steps >= max_steps:
                    self.display_message(f'Maximum steps {max_steps} exceeded')
                    return total_reward
                total_reward += float(r)
                if d:
                    self.display_message(f'Total reward: {total_reward}')
                    return total_reward
                steps += 1

    def _play_chunk(self):
        """Step every env with the play policy for one or more steps; env 0's rewards and
        dones (host arrays, one entry per step, in step order)."""
        raise NotImplementedError(f'play() is not available for {type(self).__name__}')


class OnPolicy(BaseAgent, ABC):
    def __init__(self, envs, model, **kwargs):
        super(OnPolicy, self).__init__(envs, model, **kwargs)


class OffPolicy(BaseAgent, ABC):
    def __init__(
        self,
        envs,
        model,
        buffers,
        prioritized=False,
        per_alpha=0.6,
        per_beta=0.4,
        per_beta_steps=100000,
        per_eps=1e-6,
        **kwargs,
    ):
        self._check_prioritized(prioritized)
        super(OffPolicy, self).__init__(envs, model, **kwargs)
        assert len(envs) == len(buffers), (
            f'Expected equal env and replay buffer sizes, got {self.n_envs} '
            f'and {len(buffers)}'
        )
        self.buffers = buffers
        self.prioritized = bool(prioritized)
        self.per_alpha, self.per_eps = per_alpha, per_eps
        self.per_beta = self.per_beta_start = per_beta
        self.per_beta_steps = per_beta_steps
        self.per = None  # the PrioritizedSampler, built with the rings (_setup_offpolicy)
        self.step_stats = None  # the env steps' StepStats (_setup_offpolicy)

    # ---- prioritized replay (xagents_amd/per.py) ------------------------------------
    # agents whose learner phase samples through the PrioritizedSampler (DQN, SAC)
    _supports_prioritized = False

    @classmethod
    def _check_prioritized(cls, prioritized):
        """Refuse prioritized=True where no path takes it, before anything is built."""
        if not prioritized:
            return
        if not cls._supports_prioritized:
            raise NotImplementedError(
                f'{cls.__name__} has no prioritized replay path (DQN and SAC have; the fused '
                f'DDPG / TD3 launch gathers its batch internally)')
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            raise NotImplementedError(
                'prioritized replay has no data-parallel path: every rank would need the '
                'union of the ranks\' priorities')

    def _per_anneal(self):
        """beta grows linearly from per_beta to 1 over per_beta_steps agent steps; the host
        writes it into the sampler's device scalar (outside any captured phase) when it
        moves."""
        if self.per is None:
            return
        frac = min(1.0, self.steps / self.per_beta_steps) if self.per_beta_steps > 0 else 1.0
        beta = self.per_beta_start + (1.0 - self.per_beta_start) * frac
        if beta != self.per_beta:
            self.per_beta = beta
            self.per.set_beta(beta)

    # ---- the sampled batch's slots: one learner-phase order, two slot sources ----------
    # uniform replay draws them on the host (the reference's RNG streams) before the phase is
    # enqueued; prioritized replay draws them in the phase's first launch. The phase itself is
    # the same either way: gather from _phase_slots(), the TD head with _per_ptrs(), and
    # per.update() behind it when there is a sampler.
    def _draw_slots(self, stage=None):
        """Host side, before the phase that gathers is enqueued. Uniform: sample_slots() into
        `stage` (a SlotStage the gather reads in place) or, without one, uploaded into
        replay.slots. Prioritized: nothing."""
        if self.per is None:
            slots = self.replay.sample_slots()
            if stage is not None:
                stage.put(slots)
            else:
                self.replay.upload_slots(slots)

    def _phase_slots(self, stage=None):
        """Inside the phase: the device address the gather reads its slots from (prioritized:
        behind the xa_per_sample launch that draws them)."""
        if self.per is not None:
            return self.per.sample().data_ptr()
        return stage.address(0) if stage is not None else self.replay.slots.data_ptr()

    def _per_ptrs(self):
        """(importance weights in, |TD error| out) of the weighted TD heads; null without a
        sampler, which gives the plain head's bytes."""
        if self.per is None:
            return None, None
        return self.per.weights.data_ptr(), self.per.td_abs.data_ptr()

    # ---- device env stepping + replay append (step_envs(store_in_buffers=True)) ----
    _STATS_ROWS = 64

    def _setup_offpolicy(self, act_shape, act_dtype):
        """Device replay rings mirroring self.buffers, the fused env-step arguments and
        the per-step episode-stat rows copied back asynchronously."""
        import torch.distributed as dist
        from xagents_amd._lib import XaReplayStepArgs
        from xagents_amd.episode_stats import StepStats
        from xagents_amd.replay import DeviceReplay
        # data parallel over env shards: each rank samples its own buffers, gradients
        # are all-reduced (sum) and scaled by 1 / world before Adam
        self.distributed = dist.is_available() and dist.is_initialized()
        self.world_size = dist.get_world_size() if self.distributed else 1
        self.rank = dist.get_rank() if self.distributed else 0
        # ranks sharing one GPU (the multi-process tests) split its resident-workgroup
        # capacity for the persistent kernels (DDPG / TD3 fused step): collective, so once here
        self._ranks_share = 1
        if self.distributed and torch.device(self.device).type == 'cuda':
            from xagents_amd.comm import ranks_per_device
            self._ranks_share = ranks_per_device()
        env = self.envs
        self.replay = DeviceReplay(self.buffers, env.obs_shape, env.obs_dtype, act_shape,
                                   act_dtype, self.device)
        if self.prioritized:
            from xagents_amd.per import PrioritizedSampler
            self.per = PrioritizedSampler(self.replay, self.per_alpha, self.per_beta,
                                          self.per_eps, self.seed or 0)
        self._step_args = XaReplayStepArgs()
        env.fill_step_args(self._step_args)
        self.step_stats = StepStats(self, self._STATS_ROWS)

    def _env_step(self, actions, store=True):
        """One xa_replay_env_step: every env steps with `actions` (device) and, when
        `store`, appends its transition to its replay ring (xagents/base.py:388-426)."""
        a = self._step_args
        if store:
            self.replay.fill_step_args(a, actions)
        else:
            a.ring_states = None
            a.actions, a.act_bytes = actions.data_ptr(), self.replay.act_bytes
        a.out_dones, a.done_epret = self.step_stats.ptrs[self.step_stats.row]
        if store and self.per is not None:
            self.per.mark()  # reads the ring counters before the step's append
        self.envs.step_into(a, actions)
        if store:
            self.replay.appended()
        self.step_stats.advance()

    def _play_actions(self):
        """Device actions of the play policy for every env (subclasses)."""
        raise NotImplementedError(f'play() is not available for {type(self).__name__}')

    def _play_chunk(self):
        """One xa_replay_env_step with the play policy's actions and no replay append;
        reward / done rows go to play-only buffers, so the training statistics rows and
        the rings are untouched."""
        from xagents_amd._lib import XaReplayStepArgs
        if getattr(self, '_play_args', None) is None:
            n = self.n_envs
            self._play_out = torch.zeros(3, n, dtype=torch.float32, device=self.device)
            a = XaReplayStepArgs()
            self.envs.fill_step_args(a)
            a.ring_states = None
            o = self._play_out
            a.out_rewards, a.out_dones = o[0].data_ptr(), o[1].data_ptr()
            a.done_epret = o[2].data_ptr()
            self._play_args = a
        a = self._play_args
        actions = self._play_actions()
        a.actions, a.act_bytes = actions.data_ptr(), self.replay.act_bytes
        self.envs.step_into(a, actions)
        out = self._play_out[:2, 0].cpu().numpy()
        return out[:1], out[1:]

    def _device_checks(self):
        """Raise on an error a persistent launch reported through its device status word
        (subclasses; called with every statistics flush, so no extra sync per step)."""

    def _drain_episode_stats(self):
        super()._drain_episode_stats()
        if self.step_stats is not None:
            self.step_stats.drain()

    def _sync_params(self, *models):
        if self.distributed:
            import torch.distributed as dist
            for m in models:
                dist.broadcast(m.theta, 0)

    def _reduce_grad(self, grad, mean=False):
        """All-reduce (sum) a gradient over the data-parallel ranks; returns Adam's
        grad_scale so the step equals one process on the union of the ranks' batches:
        1 for losses summed over the batch (Keras MSE + minimize: DQN, the critics,
        dqn/agent.py:170-171, ddpg/agent.py:126-127), 1 / world for batch means (the
        actor's -mean Q, ddpg/agent.py:97-100) when every rank samples the same count."""
        if not self.distributed:
            return 1.0
        import torch.distributed as dist
        dist.all_reduce(grad)
        return 1.0 / self.world_size if mean else 1.0

    def _all_gather_host(self, arr):
        """Concatenation over the ranks (rank-major) of a small host array."""
        import torch.distributed as dist
        parts = [None] * self.world_size
        dist.all_gather_object(parts, np.asarray(arr))
        return np.concatenate(parts)

    def _fill_action_plan(self):
        """The random actions of fill_buffers in the reference's draw order: env 0's
        action_space.sample() calls until its buffer is full, then env 1's, ...
        (xagents/base.py:702-730); [max missing, n_envs, *act] plus each env's count."""
        space = self.envs[0].action_space
        need = [max(b.initial_size - b.current_size, 0) for b in self.buffers]
        seqs = [[np.asarray(space.sample()) for _ in range(k)] for k in need]
        width = max(need) if need else 0
        proto = np.asarray(space.sample()) if width else None
        plan = None
        if width:
            plan = np.zeros((width, self.n_envs) + proto.shape, proto.dtype)
            for i, seq in enumerate(seqs):
                if seq:
                    plan[:len(seq), i] = np.stack(seq)
        return plan, need

    def fill_buffers(self):
        """Random actions until each buffer holds initial_size transitions
        (xagents/base.py:702-730), then reset the envs. The actions are drawn env by env
        in the reference's order (_fill_action_plan); the device then steps every env
        together (an env that needed fewer than another takes action 0 on the extra
        steps, which leaves the draw order unchanged)."""
        total = sum(b.initial_size for b in self.buffers)
        plan, need = self._fill_action_plan()
        step = 0
        while min(b.current_size - b.initial_size for b in self.buffers) < 0:
            acts = torch.as_tensor(plan[min(step, len(plan) - 1)], device=self.device)
            acts = acts.to(self.replay.act_t).contiguous()
            self._env_step(acts)
            step += 1
            filled = sum(min(b.current_size, b.initial_size) for b in self.buffers)
            complete = round((filled / total) * 100, self.display_precision)
            self.display_message(
                f'\rFilling replay buffer ==> {complete}% | {filled}/{total}', end='')
        self.display_message('')
        self._drain_episode_stats()
        self.total_rewards.clear()
        self.games = self.done_envs = 0
        self.reset_envs()

    def fit(self, target_reward=None, max_steps=None, monitor_session=None):
        self.fill_buffers()
        super(OffPolicy, self).fit(target_reward, max_steps, monitor_session)
