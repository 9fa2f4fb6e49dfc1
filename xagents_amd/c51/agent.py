"""Categorical DQN (C51) on DQN's device path (NOT a parity mode: the reference has no
distributional agent).

The Q network emits A * K logits, action-major: output a * K + i is atom i of action a on the
fixed support z_i = v_min + i (v_max - v_min) / (K - 1), p(a) is the softmax of action a's
logits and Q[a] = sum_i p_i(a) z_i. Against DQN's train step only the two head launches
differ:
    get_actions          epsilon-greedy on the expected Q                    -> xa_c51_act
    _td_grad             logits(s), [logits(s')], target logits(s') -> a* from the expected
                         Q of s', the projected target distribution m, the cross-entropy
                         -sum_i m_i log p_i(s, a) and the gradient of the batch-mean loss
                                                                             -> xa_c51_td_grad
Everything else is DQN's: the rings and the slot staging, the layer executor's backward with
its fused Adam, the captured learner phase, the target sync, prioritized replay (the priority
is the TD error of the means, so per_eps keeps DQN's units), n-step targets (n_steps > 1:
DQN's gather, the head takes each sample's gamma^m). What it shares with QRDQN is
dqn/wide.py's.
"""
import math

import torch

from xagents_amd import kernels
from xagents_amd._lib import call, stream
from xagents_amd.dqn.wide import WideHeadDQN
from xagents_amd.layers import LayerExecutor


class C51(WideHeadDQN):
    """A Distributional Perspective on Reinforcement Learning
    https://arxiv.org/abs/1707.06887

    n_atoms: K (2 .. 256), the model's single output has n_actions * K units
    (create_model(..., 'c51', ..., n_atoms=K)); v_min < v_max: the support's finite ends.
    double / prioritized / n_steps and DQN's other arguments keep their meaning; huber_delta
    has none (the loss is a cross-entropy)."""

    _width_arg, _agent_id = 'n_atoms', 'c51'

    def __init__(self, envs, model, buffers, n_atoms=51, v_min=-10.0, v_max=10.0, **kwargs):
        if 'huber_delta' in kwargs:
            raise TypeError('C51 minimizes a cross-entropy and takes no huber_delta')
        if not 2 <= int(n_atoms) <= 256:
            raise ValueError(f'n_atoms must be in 2 .. 256, got {n_atoms}')
        # (as the f32 values the kernels are handed)
        lo, hi = float(kernels._f32(v_min).value), float(kernels._f32(v_max).value)
        if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo and math.isfinite(hi - lo)):
            raise ValueError(f'the support needs finite v_min < v_max, got {v_min}, {v_max}')
        self.n_atoms = int(n_atoms)
        self.v_min, self.v_max = lo, hi
        super(C51, self).__init__(envs, model, buffers, **kwargs)

    def _support(self):
        return self.n_actions, self.n_atoms, kernels._f32(self.v_min), kernels._f32(self.v_max)

    def _act(self, logits, n, actions, q=None, random_actions=None):
        call('xa_c51_act', None if logits is None else logits.data_ptr(), n, *self._support(),
             None if random_actions is None else random_actions.data_ptr(),
             int(random_actions is not None), actions.data_ptr(),
             None if q is None else q.data_ptr(), stream())

    # ---- learner phase -------------------------------------------------------------
    def _td_grad(self):
        """The projected target distribution + the cross-entropy gradient in one launch, which
        also bumps the optimizer's t (the update's Adam reads it after the backward)."""
        B = self.batch_size
        lg_all = self.ex_online.forward(self.xb if self.double else self.xb[:B])[0]
        lg_next_t = self.ex_target.forward(self.xb[B:])[0]
        lg_next_o = lg_all[B:].data_ptr() if self.double else None
        disc = self.b_disc.data_ptr() if self.n_steps > 1 else None
        call('xa_c51_td_grad', lg_all.data_ptr(), lg_next_t.data_ptr(), lg_next_o, None,
             self.b_act.data_ptr(), self.b_rew.data_ptr(), self.b_done.data_ptr(), B,
             *self._support(), kernels._f32(self.gamma), self.dq.data_ptr(),
             self.td_loss.data_ptr(), self.model.optimizer.iterations.data_ptr(),
             *self._per_ptrs(), disc, stream())

    # ---- composed path (a subclass that overrides a hook) ----------------------------
    def get_targets(self, states, actions, rewards, dones, new_states):
        """The projected target distribution m [B, K] (xa_c51_project): a* the greedy action
        of the target net's expected Q on s' (the online net's when double)."""
        B = new_states.shape[0]
        lg_t = self._outputs(new_states, self.target_model)
        lg_o = self._outputs(new_states, self.model) if self.double else None
        r = torch.as_tensor(rewards, device=self.device).float().contiguous()
        d = torch.as_tensor(dones, device=self.device).float().contiguous()
        m = torch.empty(B, self.n_atoms, dtype=torch.float32, device=self.device)
        call('xa_c51_project', lg_t.data_ptr(), None if lg_o is None else lg_o.data_ptr(),
             r.data_ptr(), d.data_ptr(), None, B, *self._support(), kernels._f32(self.gamma),
             m.data_ptr(), stream())
        return m

    def update_gradients(self, x, m, actions=None):
        """The cross-entropy of the given target distributions m [B, K] at `actions` (default:
        the batch concat_buffer_samples gathered last), minimized with Keras Adam. The head
        launch is the fused path's, reading m instead of projecting."""
        x = torch.as_tensor(x, device=self.device).contiguous()
        m = torch.as_tensor(m, device=self.device, dtype=torch.float32).contiguous()
        B = x.shape[0]
        act = self.b_act if actions is None else torch.as_tensor(
            actions, device=self.device).to(torch.int32).contiguous()
        ex = LayerExecutor(self.model, B)
        logits = ex.forward(x)[0]
        dq = torch.empty_like(logits)
        call('xa_c51_td_grad', logits.data_ptr(), None, None, m.data_ptr(), act.data_ptr(),
             None, None, B, *self._support(), kernels._f32(self.gamma), dq.data_ptr(), None,
             self.model.optimizer.iterations.data_ptr(), None, None, None, stream())
        self._composed_apply(ex, dq)

    def train_step(self):
        if self._hooks_overridden(C51):
            self._composed_step()
        else:
            self._device_step()
