"""What the distributional agents (QRDQN, C51) share on DQN's device path: a Q network that
emits n_actions * W outputs, action-major (W values describe one action's return: quantiles,
atom logits), a head kernel pair of their own -- the greedy action of the value the W outputs
stand for, and the TD head that writes the whole [B, A W] gradient -- and DQN's everything
else. A subclass names its width, gives `_act` (its act launch) and `_td_grad`, and keeps
its own `train_step` (the class whose hooks choose between the two step bodies is its own).
"""
import numpy as np
import torch

from xagents_amd import kernels
from xagents_amd.dqn.agent import DQN
from xagents_amd.layers import LayerExecutor


class WideHeadDQN(DQN):
    """DQN with W outputs per action. `_width_arg` names the attribute that holds W, which is
    also create_model's argument of that name for the registry id `_agent_id`."""

    _supports_prioritized = True
    _width_arg = None
    _agent_id = None

    def _act(self, outputs, n, actions, q=None, random_actions=None):
        """The act launch: actions [n] = greedy on `outputs` [n, A W] (q [n, A] receives the
        action values), or a copy of random_actions (outputs is then None)."""
        raise NotImplementedError

    def _setup_device(self):
        arg, per_action = self._width_arg, getattr(self, self._width_arg)
        name, agent_id = self._agent_id.upper(), self._agent_id
        width = self.n_actions * per_action
        outs = list(self.model.outputs)
        units = [self.model.layers[i].units for i in outs]
        assert units == [width], (
            f'{name} needs a model with one output of n_actions * {arg} = '
            f'{self.n_actions} * {per_action} = {width} units, got {units} '
            f'(create_model(..., \'{agent_id}\', ..., {arg}={per_action}))')
        super(WideHeadDQN, self)._setup_device()
        dev = self.device
        self.dq = torch.zeros(self.batch_size, width, dtype=torch.float32, device=dev)
        self.q_mean = torch.zeros(self.n_envs, self.n_actions, dtype=torch.float32, device=dev)

    def _head_fused(self):
        """Never: xa_dqn_head is the scalar-Q head on a row-dot layer of <= 8 outputs."""
        return False

    # ---- acting --------------------------------------------------------------------
    def get_model_outputs(self, inputs, models, training=True):
        """[greedy action, action values [n, A]] for a device batch of states."""
        model = models[0] if isinstance(models, (list, tuple)) else models
        x = torch.as_tensor(inputs, device=self.device).contiguous()
        n = x.shape[0]
        out = LayerExecutor(model, n).forward(x)[0]
        act = torch.empty(n, dtype=torch.int32, device=self.device)
        q = torch.empty(n, self.n_actions, dtype=torch.float32, device=self.device)
        self._act(out, n, act, q)
        return act, q

    def get_actions(self):
        """Epsilon-greedy on the action values, the host draws DQN's (all envs random or all
        greedy)."""
        if np.random.random() < self.epsilon:
            r = np.random.randint(0, self.n_actions, self.n_envs)
            self._rand_actions.copy_(torch.from_numpy(r.astype(np.int32)))
            self._act(None, self.n_envs, self.actions, random_actions=self._rand_actions)
        else:
            self._play_actions()
        return self.actions

    def _play_actions(self):
        """play(): the greedy action for every env (the action values at self.q_mean)."""
        out = self.ex_act.forward(self.envs.state)[0]
        self._act(out, self.n_envs, self.actions, self.q_mean)
        return self.actions

    # ---- composed path (a subclass that overrides a hook) ----------------------------
    def _outputs(self, states, model):
        x = torch.as_tensor(states, device=self.device).contiguous()
        return LayerExecutor(model, x.shape[0]).forward(x)[0].clone()

    def _composed_apply(self, ex, dq):
        """update_gradients' tail: the backward of the head gradient dq through the executor
        that ran the forward, then Keras Adam (the head launch bumped t)."""
        opt = self.model.optimizer
        ex.backward([dq], self.grad)
        kernels.clip_adam(self.model.theta, opt.m, opt.v, self.grad, opt.iterations,
                          opt.learning_rate, opt.beta_1, opt.beta_2, opt.epsilon,
                          clip_norm=0.0, workspace=self.adam_ws)

    def _composed_step(self):
        """DQN's, with the sampled actions handed to update_gradients."""
        self._refuse_composed_nstep()
        actions = self.get_actions()
        self._env_step(actions.to(torch.int32).contiguous())
        self.steps += self.n_envs
        batch = self.concat_buffer_samples()
        self.update_gradients(batch[0], self.get_targets(*batch), batch[1])
