"""Soft Actor-Critic on the device path: TD3's replay, twin critics, Keras Adam and captured
phases with a stochastic tanh-squashed Gaussian policy, the entropy-regularised critic
target and a learned temperature (csrc/sac.hip, arithmetic in csrc/sac_terms.hpp).

Per gradient step, two captured phases:
    critic  gather -> actor(s') -> xa_sac_sample (a', logp') -> both target critics on
            [s', a'] -> both critics on [s, a] -> xa_sac_td_grad -> backward -> Adam x 2
    actor   actor(s) -> xa_sac_sample (a_pi, eps, logp) -> both UPDATED critics on [s, a_pi]
            -> xa_sac_actor_seed -> both critic input gradients (summed) -> xa_sac_head_grad
            -> actor backward from [dmean, dlog_std] -> Adam -> (alpha='auto') Adam on
            log_alpha -> xa_polyak of both critics
alpha = exp(log_alpha) is read on device by every launch; the temperature step comes last, so
every launch of a gradient step saw the same alpha. There is no target actor and no fused
single-launch step.

prioritized=True (per.py; not a parity mode): the sampler is the critic phase's slot source.
"""
import numpy as np
import torch

from xagents_amd import kernels
from xagents_amd._lib import call, stream
from xagents_amd.layers import LayerExecutor
from xagents_amd.nets import Adam
from xagents_amd.td3.agent import TD3


class Temperature:
    """log_alpha as a one-parameter model: theta [1] with Keras Adam state (SAC.save_weights
    stores it in the actor's .npz)."""

    def __init__(self, initial_alpha, learning_rate, device):
        self.device = torch.device(device)
        self.n_params = 1
        self.theta = torch.full((1,), float(np.log(initial_alpha)), dtype=torch.float32,
                                device=self.device)
        self.optimizer = Adam(learning_rate=learning_rate)
        self.optimizer.bind(1, self.device)


class SAC(TD3):
    """Soft Actor-Critic Algorithms and Applications https://arxiv.org/abs/1812.05905

    prioritized / per_alpha / per_beta / per_beta_steps / per_eps (OffPolicy): proportional
    prioritized replay, sampled on the device; the critics' gradients carry the importance
    weights, the priority is the twins' mean |TD error|. beta anneals linearly to 1 over
    per_beta_steps agent steps. Not a parity mode: the host RNG streams are not consumed by
    the draw. The batch's weights are at agent.per.weights."""

    _supports_prioritized = True

    def __init__(
        self,
        envs,
        actor_model,
        critic_model,
        buffers,
        gradient_steps=None,
        tau=0.005,
        alpha='auto',
        initial_alpha=1.0,
        target_entropy=None,
        alpha_learning_rate=None,
        huber_delta=None,
        **kwargs,
    ):
        import torch.distributed as dist
        self.data_parallel = kwargs.pop('data_parallel', None)
        if dist.is_available() and dist.is_initialized() and self.data_parallel is not False:
            raise NotImplementedError(
                'SAC has no data-parallel path: pass data_parallel=False to train one '
                'independent agent per process')
        self._check_prioritized(kwargs.get('prioritized', False))
        assert alpha == 'auto' or float(alpha) > 0, f"alpha is 'auto' or positive, got {alpha}"
        assert len(actor_model.outputs) == 2, (
            f'The SAC actor has two outputs [mean, log_std], got {len(actor_model.outputs)}')
        self.auto_alpha = alpha == 'auto'
        self._alpha0 = float(initial_alpha if self.auto_alpha else alpha)
        self._alpha_lr = alpha_learning_rate
        self._target_entropy = target_entropy
        super(SAC, self).__init__(envs, actor_model, critic_model, buffers, policy_delay=1,
                                  gradient_steps=gradient_steps, tau=tau, step_noise_coef=0.0,
                                  huber_delta=huber_delta, **kwargs)
        # no target actor: the next action comes from the current policy
        del self.target_actor, self.ex_target_actor
        self.model_groups = [(self.critic1, self.target_critic1),
                             (self.critic2, self.target_critic2)]
        self._setup_sac()

    def _setup_offpolicy(self, act_shape, act_dtype):
        super()._setup_offpolicy(act_shape, act_dtype)
        # data_parallel=False inside an initialised process group: an independent agent
        self.distributed, self.world_size, self._ranks_share = False, 1, 1

    def _setup_sac(self):
        B, A, n = self.batch_size, self.A, self.n_envs
        for i in self.actor.outputs:
            units = self.actor.layers[i].units
            assert units == A, f'Expected actor outputs of {A} units, got {units}'
        f32 = dict(dtype=torch.float32, device=self.device)
        self.target_entropy = float(-A if self._target_entropy is None else self._target_entropy)
        lr = self._alpha_lr if self._alpha_lr is not None else self.actor.optimizer.learning_rate
        self.temperature = Temperature(self._alpha0, lr, self.device)
        self.log_alpha = self.temperature.theta
        self.g_log_alpha = torch.zeros(1, **f32)
        # parity surface: the draws and log-densities of a' (next) and a_pi
        self.eps, self.eps_next = torch.zeros(B, A, **f32), torch.zeros(B, A, **f32)
        self.logp, self.logp_next = torch.zeros(B, **f32), torch.zeros(B, **f32)
        self.dq1, self.dq2 = torch.zeros(B, 1, **f32), torch.zeros(B, 1, **f32)
        self.actor_loss = torch.zeros(B, **f32)
        self.dmean, self.dlog_std = torch.zeros(B, A, **f32), torch.zeros(B, A, **f32)
        self.play_actions = torch.zeros(n, A, **f32)
        self.ex_critic2_pi = LayerExecutor(self.critic2, B)

    @property
    def alpha(self):
        return float(np.exp(self.log_alpha.item()))

    # ---- the persistent TD3 launches are not SAC's ---------------------------------
    def _fused_args(self):
        return None

    def _fused_act_args(self):
        return None

    # ---- policy head -----------------------------------------------------------------
    def _sample(self, heads, out, ld_out, deterministic=False, eps_out=None, logp=None):
        """xa_sac_sample of the actor outputs `heads` = [mean, log_std] into `out` (row
        stride ld_out floats); a draw advances the Philox counter, as DDPG._noisy does."""
        mean, log_std = heads
        rows, A = mean.shape
        call('xa_sac_sample', mean.data_ptr(), A, log_std.data_ptr(), A, rows, A, None,
             self.rng_counter.data_ptr(), self.rng_seed, int(deterministic), out, ld_out,
             eps_out.data_ptr() if eps_out is not None else None,
             logp.data_ptr() if logp is not None else None, stream())
        if not deterministic:
            kernels.counter_bump(self.rng_counter)

    def _policy_inputs(self, ex, states, out, eps_out, logp):
        """[states, a] into `out`, a ~ pi(states) through executor `ex`; returns its heads."""
        S, A = self.S, self.A
        heads = ex.forward(states)
        call('xa_copy_block', states.data_ptr(), S, out.data_ptr(), S + A, self.batch_size, S,
             stream())
        self._sample(heads, out.data_ptr() + 4 * S, S + A, eps_out=eps_out, logp=logp)
        return heads

    def get_step_actions(self):
        """a = tanh(mean + exp(log_std) eps) of the env states, in [-1, 1] (the env clips to
        its own bound)."""
        heads = self.ex_step.forward(self.envs.state)
        self._sample(heads, self.step_actions.data_ptr(), self.A)
        return self.step_actions

    def _play_actions(self):
        """play(): the policy's mode tanh(mean), nothing drawn."""
        heads = self.ex_step.forward(self.envs.state)
        self._sample(heads, self.play_actions.data_ptr(), self.A, deterministic=True)
        return self.play_actions

    # ---- gradient step ---------------------------------------------------------------
    def update_critic_weights(self, states=None, actions=None, new_states=None, dones=None,
                              rewards=None):
        """Both critics against r + (1 - d) gamma (min target Q(s', a') - alpha logp'),
        a' ~ pi(s')."""
        self._policy_inputs(self.ex_actor, self.s2, self.s2a2, self.eps_next, self.logp_next)
        tv1 = self.ex_target_critic.forward(self.s2a2)[0]
        tv2 = self.ex_target_critic2.forward(self.s2a2)[0]
        self._concat(self.s, self.a, self.sa)
        v1 = self.ex_critic.forward(self.sa)[0]
        v2 = self.ex_critic2.forward(self.sa)[0]
        # (null weights: xa_sac_td_grad's bytes)
        call('xa_sac_td_grad_w', v1.data_ptr(), v2.data_ptr(), tv1.data_ptr(), tv2.data_ptr(),
             self.logp_next.data_ptr(), self.log_alpha.data_ptr(), self.r.data_ptr(),
             self.d.data_ptr(), self.batch_size, kernels._f32(self.gamma),
             kernels._f32(self.huber_delta or 0.0), self.dv1.data_ptr(), self.dv2.data_ptr(),
             self.critic_loss.data_ptr(), *self._per_ptrs(), stream())
        if self.per is not None:
            self.per.update()
        self.ex_critic.backward([self.dv1], self.g_critic)
        self.ex_critic2.backward([self.dv2], self.g_critic2)
        self._adam(self.critic1, self.g_critic)
        self._adam(self.critic2, self.g_critic2)

    def update_actor_weights(self, states=None):
        """mean(alpha logp - min Q(s, a_pi)) minimised over the actor through both updated
        critics; the temperature gradient -mean(logp + target_entropy) on the way."""
        B, S, A = self.batch_size, self.S, self.A
        heads = self._policy_inputs(self.ex_actor, self.s, self.spa, self.eps, self.logp)
        q1 = self.ex_critic_pi.forward(self.spa)[0]
        q2 = self.ex_critic2_pi.forward(self.spa)[0]
        call('xa_sac_actor_seed', q1.data_ptr(), q2.data_ptr(), self.logp.data_ptr(),
             self.log_alpha.data_ptr(), B, kernels._f32(self.target_entropy),
             self.dq1.data_ptr(), self.dq2.data_ptr(), self.actor_loss.data_ptr(),
             self.g_log_alpha.data_ptr(), stream())
        self.ex_critic_pi.backward([self.dq1], None, dinput=self.dspa)
        self.ex_critic2_pi.backward([self.dq2], None, dinput=self.dspa, dinput_accumulate=True)
        call('xa_sac_head_grad', self.dspa.data_ptr() + 4 * S, S + A,
             self.spa.data_ptr() + 4 * S, S + A, self.eps.data_ptr(), heads[1].data_ptr(), A,
             self.log_alpha.data_ptr(), B, A, self.dmean.data_ptr(), self.dlog_std.data_ptr(),
             stream())
        self.ex_actor.backward([self.dmean, self.dlog_std], self.g_actor)
        self._adam(self.actor, self.g_actor, mean=True)

    def update_temperature(self):
        """One Keras Adam step on log_alpha from xa_sac_actor_seed's gradient."""
        self._adam(self.temperature, self.g_log_alpha, mean=True)

    def at_step_start(self):
        self._per_anneal()

    def _actor_phase(self):
        self.update_actor_weights()
        if self.auto_alpha:
            self.update_temperature()
        self.sync_target_models()

    # ---- checkpoints -----------------------------------------------------------------
    def _checkpoint_extras(self):
        """What the three model files carry beside their own model (extra .npz keys, which
        DeviceModel.load_weights ignores): each critic file its target, the actor file the
        temperature."""
        return [[('log_alpha', self.temperature)], [('target', self.target_critic1)],
                [('target', self.target_critic2)]]

    def save_weights(self, paths):
        """One .npz per output model (actor, critic 1, critic 2), as the other agents'
        checkpoints, plus the targets and log_alpha with its Adam moments and step count."""
        from pathlib import Path
        assert len(paths) == len(self.output_models), (
            f'Expected {len(self.output_models)} checkpoints, got {len(paths)}')
        for model, path, extras in zip(self.output_models, paths, self._checkpoint_extras()):
            opt = model.optimizer
            state = {'theta': model.theta.detach().cpu().numpy(),
                     'adam_m': opt.m.cpu().numpy(), 'adam_v': opt.v.cpu().numpy(),
                     'adam_t': opt.iterations.cpu().numpy()}
            for name, extra in extras:
                state[f'{name}_theta'] = extra.theta.detach().cpu().numpy()
                opt = getattr(extra, 'optimizer', None)
                if opt is not None:
                    state[f'{name}_adam_m'] = opt.m.cpu().numpy()
                    state[f'{name}_adam_v'] = opt.v.cpu().numpy()
                    state[f'{name}_adam_t'] = opt.iterations.cpu().numpy()
            np.savez(Path(path), **state)

    def load_weights(self, paths):
        from pathlib import Path
        assert len(paths) == len(self.output_models), (
            f'Expected {len(self.output_models)} weights to load, got {len(paths)}')
        for model, path, extras in zip(self.output_models, paths, self._checkpoint_extras()):
            model.load_weights(path)
            p = Path(path)
            if not p.exists():
                p = p.with_suffix(p.suffix + '.npz')
            with np.load(p, allow_pickle=False) as data:
                for name, extra in extras:
                    if f'{name}_theta' not in data:
                        # a plain model file: the target restarts from its model
                        if name == 'target':
                            extra.theta.copy_(model.theta)
                        continue
                    dev = lambda k: torch.from_numpy(data[f'{name}_{k}']).to(self.device)  # noqa: E731
                    extra.theta.copy_(dev('theta'))
                    opt = getattr(extra, 'optimizer', None)
                    if opt is not None and f'{name}_adam_m' in data:
                        opt.m.copy_(dev('adam_m'))
                        opt.v.copy_(dev('adam_v'))
                        opt.iterations.copy_(dev('adam_t'))
        return self

    def checkpoint(self):
        """BaseAgent.checkpoint with the agent's own save (targets and temperature too)."""
        if self.mean_reward > self.best_reward:
            self.plateau_count = 0
            self.early_stop_count = 0
            self.display_message(
                f'Best reward updated: {self.best_reward} -> {self.mean_reward}')
            if self.checkpoints:
                self.save_weights(self.checkpoints)
        self.best_reward = max(self.mean_reward, self.best_reward)
