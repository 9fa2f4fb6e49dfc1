"""Quantile-regression DQN on DQN's device path (NOT a parity mode: the reference has no
distributional agent).

The Q network emits A * N outputs, action-major: output a * N + i is quantile i of action a
at the midpoint (2 i + 1) / (2 N), and Q[a] is their mean. Against DQN's train step only the
two head launches differ:
    get_actions          epsilon-greedy on the mean Q                        -> xa_qr_act
    _td_grad             Q(s), [Q(s')], Qt(s') -> a* from the mean Q of s', the N target
                         quantiles, the N x N quantile-Huber terms and the gradient of the
                         batch-mean loss                                     -> xa_qr_td_grad
Everything else is DQN's: the rings and the slot staging, the layer executor's backward with
its fused Adam, the captured learner phase, the target sync, prioritized replay (the priority
is the TD error of the means, so per_eps keeps DQN's units), n-step targets (n_steps > 1:
DQN's gather, and xa_qr_td_grad_n takes each sample's gamma^m).
"""
import numpy as np
import torch

from xagents_amd import kernels
from xagents_amd._lib import call, stream
from xagents_amd.dqn.wide import WideHeadDQN
from xagents_amd.layers import LayerExecutor


class QRDQN(WideHeadDQN):
    """Distributional Reinforcement Learning with Quantile Regression
    https://arxiv.org/abs/1710.10044

    n_quantiles: N (1 .. 256), the model's single output has n_actions * N units
    (create_model(..., 'qrdqn', ..., n_quantiles=N)). huber_kappa > 0: the quantile Huber
    loss's threshold (the discontinuous pinball loss, kappa = 0, has no path here).
    double / prioritized and DQN's other arguments keep their meaning; huber_delta has none."""

    _width_arg, _agent_id = 'n_quantiles', 'qrdqn'

    def __init__(self, envs, model, buffers, n_quantiles=32, huber_kappa=1.0, **kwargs):
        if 'huber_delta' in kwargs:
            raise TypeError('QRDQN takes huber_kappa (the quantile Huber threshold), not '
                            'huber_delta')
        if not huber_kappa > 0:
            raise ValueError(f'huber_kappa must be > 0, got {huber_kappa}')
        if not 1 <= int(n_quantiles) <= 256:
            raise ValueError(f'n_quantiles must be in 1 .. 256, got {n_quantiles}')
        self.n_quantiles = int(n_quantiles)
        self.huber_kappa = float(huber_kappa)
        super(QRDQN, self).__init__(envs, model, buffers, **kwargs)

    def _act(self, theta, n, actions, q=None, random_actions=None):
        call('xa_qr_act', None if theta is None else theta.data_ptr(), n, self.n_actions,
             self.n_quantiles, None if random_actions is None else random_actions.data_ptr(),
             int(random_actions is not None), actions.data_ptr(),
             None if q is None else q.data_ptr(), stream())

    # ---- learner phase -------------------------------------------------------------
    def _td_grad(self):
        """Target quantiles + the quantile-Huber gradient; the same launch bumps the
        optimizer's t (the update's Adam reads it after the backward)."""
        B = self.batch_size
        th_all = self.ex_online.forward(self.xb if self.double else self.xb[:B])[0]
        th_next_t = self.ex_target.forward(self.xb[B:])[0]
        th_next_o = th_all[B:].data_ptr() if self.double else None
        name, disc = self._td_entry('xa_qr_td_grad', 'xa_qr_td_grad_n')
        call(name, th_all.data_ptr(), th_next_t.data_ptr(), th_next_o,
             self.b_act.data_ptr(), self.b_rew.data_ptr(), self.b_done.data_ptr(), B,
             self.n_actions, self.n_quantiles, kernels._f32(self.gamma),
             kernels._f32(self.huber_kappa), self.dq.data_ptr(), self.td_loss.data_ptr(),
             self.model.optimizer.iterations.data_ptr(), *self._per_ptrs(), *disc, stream())

    # ---- composed path (a subclass that overrides a hook) ----------------------------
    def get_targets(self, states, actions, rewards, dones, new_states):
        """Target quantiles y [B, N]: theta_target(s')[a*] gamma + r, r where done, a* the
        greedy action of the target net's mean Q on s' (the online net's when double)."""
        B, N = new_states.shape[0], self.n_quantiles
        th_t = self._outputs(new_states, self.target_model).view(B, self.n_actions, N)
        a_next = self.get_model_outputs(
            new_states, self.model if self.double else self.target_model)[0].long()
        v = th_t[torch.arange(B, device=self.device), a_next]
        d = torch.as_tensor(dones, device=self.device).bool()
        v = torch.where(d[:, None], torch.zeros_like(v), v)
        r = torch.as_tensor(rewards, device=self.device).float()
        return v * np.float32(self.gamma) + r[:, None]

    def update_gradients(self, x, y, actions=None):
        """The quantile-Huber loss of the given target quantiles y [B, N] at `actions`
        (default: the batch concat_buffer_samples gathered last), minimized with Keras Adam.
        The head launch is the fused path's: y stands as every action's next-state row with
        done = 0, gamma = 1 and r = 0, which hands y_j back bit for bit whatever a* is."""
        x = torch.as_tensor(x, device=self.device).contiguous()
        y = torch.as_tensor(y, device=self.device, dtype=torch.float32)
        B, A, N = x.shape[0], self.n_actions, self.n_quantiles
        act = self.b_act if actions is None else torch.as_tensor(
            actions, device=self.device).to(torch.int32).contiguous()
        ex = LayerExecutor(self.model, B)
        theta = ex.forward(x)[0]
        dq = torch.empty_like(theta)
        y_rows = y.reshape(B, 1, N).expand(B, A, N).contiguous()
        zeros = torch.zeros(B, dtype=torch.float32, device=self.device)
        opt = self.model.optimizer
        call('xa_qr_td_grad', theta.data_ptr(), y_rows.data_ptr(), None, act.data_ptr(),
             zeros.data_ptr(), zeros.data_ptr(), B, A, N, kernels._f32(1.0),
             kernels._f32(self.huber_kappa), dq.data_ptr(), None, opt.iterations.data_ptr(),
             None, None, stream())
        self._composed_apply(ex, dq)

    def train_step(self):
        if self._hooks_overridden(QRDQN):
            self._composed_step()
        else:
            self._device_step()
