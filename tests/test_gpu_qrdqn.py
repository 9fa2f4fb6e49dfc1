"""GPU tests of quantile-regression DQN (xagents_amd/qrdqn, csrc/qr.hip): both kernels against
the float64 restatement (tests/qr_ref.py) at its fixed shapes, the weighted head bit for bit,
and the agent -- one train step against the f64 network oracle seeded with the restatement's
dtheta, the captured learner phase, prioritized replay, fit, play, checkpoints, the composed
path.

Tolerances:
* kernels: qr_ref.bounds, derived there from the arithmetic (no figure is taken from a run);
  the greedy actions are compared exactly (the generator keeps every compared pair of mean-Q
  values 1e-3 apart).
* raw gradients through the layer executor: the project's 1e-4 relative
  (tests/test_gpu_scale.py); the Adam step in test_dqn_train_step_vs_f64's form.
"""
import functools
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import qr_ref as R

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / 'oracle'))
pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4
GAMMA = np.float32(R.GAMMA)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.linalg.norm(np.asarray(got, np.float64) - want) /
                 max(np.linalg.norm(want), 1e-30))


def _dev(device, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _call(name, *args):
    from xagents_amd._lib import call, stream
    call(name, *args, stream())
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _case(B, A, N, kappa):
    """The fixed inputs and their float64 results (plain and double), computed once."""
    c = R.case(B, A, N, kappa)
    ref = {d: R.td(c['theta'], c['next_t'], c['next_o'] if d else None, c['act'], c['rew'],
                   c['done'], R.GAMMA, kappa, A, N) for d in (False, True)}
    return c, ref, R.bounds(c, kappa)


def _td(device, c, kappa, double, weights=None, td_abs=None, adam_step=None, N=None,
        want_loss=True):
    """xa_qr_td_grad on a case; outputs carry a guard row that must stay untouched."""
    B, A = c['B'], c['A']
    N = N or c['N']
    t = {k: _dev(device, c[k]) for k in ('theta', 'next_t', 'next_o', 'act', 'rew', 'done')}
    d = torch.full((B + 1, A * c['N']), 7.0, device=device)
    loss = torch.full((B + 1,), 7.0, device=device)
    _call('xa_qr_td_grad', t['theta'].data_ptr(), t['next_t'].data_ptr(),
          t['next_o'].data_ptr() if double else None, t['act'].data_ptr(), t['rew'].data_ptr(),
          t['done'].data_ptr(), B, A, N, float(GAMMA), float(kappa), d.data_ptr(),
          loss.data_ptr() if want_loss else None,
          None if adam_step is None else adam_step.data_ptr(),
          None if weights is None else weights.data_ptr(),
          None if td_abs is None else td_abs.data_ptr())
    d, loss = d.cpu().numpy(), loss.cpu().numpy()
    assert (d[B] == 7.0).all() and loss[B] == 7.0
    return d[:B], loss[:B]


# ---- 1. kernels against the restatement ---------------------------------------------------
@pytest.mark.parametrize('B,A,N', R.SHAPES)
def test_qr_act(device, B, A, N):
    c, _, bound = _case(B, A, N, 1.0)
    for key in ('theta', 'next_o'):
        theta = _dev(device, c[key])
        act = torch.full((B + 1,), -7, dtype=torch.int32, device=device)
        q = torch.full((B + 1, A), 7.0, device=device)
        _call('xa_qr_act', theta.data_ptr(), B, A, N, None, 0, act.data_ptr(), q.data_ptr())
        act, q = act.cpu().numpy(), q.cpu().numpy()
        assert act[B] == -7 and (q[B] == 7.0).all()
        np.testing.assert_array_equal(act[:B], R.greedy(c[key], A, N))
        err = np.abs(q[:B] - R.mean_q(c[key], A, N)).max()
        print(f'q_mean err {err:.3e} bound {bound["q_mean"]:.3e}')
        assert err <= bound['q_mean']
        # without q_mean: the same actions
        act2 = torch.full((B + 1,), -7, dtype=torch.int32, device=device)
        _call('xa_qr_act', theta.data_ptr(), B, A, N, None, 0, act2.data_ptr(), None)
        np.testing.assert_array_equal(act2.cpu().numpy()[:B], act[:B])
    # use_random copies the given actions (and reads no theta)
    given = _dev(device, np.random.default_rng(B).integers(0, A, B).astype(np.int32))
    out = torch.full((B + 1,), -7, dtype=torch.int32, device=device)
    _call('xa_qr_act', None, B, A, N, given.data_ptr(), 1, out.data_ptr(), None)
    out = out.cpu().numpy()
    assert out[B] == -7 and out[:B].tobytes() == given.cpu().numpy().tobytes()


@pytest.mark.parametrize('kappa', R.KAPPAS)
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('B,A,N', R.SHAPES)
def test_qr_td_grad(device, B, A, N, double, kappa):
    c, ref, bound = _case(B, A, N, kappa)
    want = ref[double]
    step = torch.full((2,), 41, dtype=torch.int32, device=device)
    td_abs = torch.full((B + 1,), 7.0, device=device)
    d, loss = _td(device, c, kappa, double, td_abs=td_abs, adam_step=step)
    assert step.cpu().numpy().tolist() == [42, 41]
    td = td_abs.cpu().numpy()
    assert td[B] == 7.0
    off = np.ones((B, A, N), bool)
    off[np.arange(B), c['act']] = False
    assert (d.reshape(B, A, N)[off] == 0).all()
    e_g = np.abs(d - want['dtheta']).max()
    e_l = np.abs(loss - want['loss']).max()
    e_t = np.abs(td[:B] - want['td_abs']).max()
    print(f'grad err {e_g:.3e} bound {bound["grad"]:.3e} (x B: {e_g * B:.3e}); '
          f'loss err {e_l:.3e} bound {bound["loss"]:.3e}; '
          f'td_abs err {e_t:.3e} bound {bound["td_abs"]:.3e}')
    assert np.abs(want['dtheta']).max() > 1e-3 / (B * N)
    assert e_g <= bound['grad']
    assert e_l <= bound['loss']
    assert e_t <= bound['td_abs']


# ---- 2. weights ------------------------------------------------------------------------------
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('B,A,N', [(5, 2, 63), (65, 6, 2), (5, 6, 256)])
def test_qr_td_head_weights(device, B, A, N, double):
    kappa = 0.25
    c, ref, bound = _case(B, A, N, kappa)
    d0, loss0 = _td(device, c, kappa, double)
    d1, loss1 = _td(device, c, kappa, double)  # null weights twice: the same bytes
    assert d1.tobytes() == d0.tobytes() and loss1.tobytes() == loss0.tobytes()
    w = c['weights']
    td_abs = torch.full((B + 1,), 7.0, device=device)
    d2, loss2 = _td(device, c, kappa, double, weights=_dev(device, w), td_abs=td_abs)
    assert d2.tobytes() == (d0 * w[:, None]).tobytes()
    assert loss2.tobytes() == (loss0 * w).tobytes()
    # td_abs is not weighted, and asking for it changes nothing else
    td = td_abs.cpu().numpy()
    assert td[B] == 7.0 and np.abs(td[:B] - ref[double]['td_abs']).max() <= bound['td_abs']
    d3, _ = _td(device, c, kappa, double, want_loss=False)
    assert d3.tobytes() == d0.tobytes()


# ---- 3. illegal shapes -----------------------------------------------------------------------
def test_illegal_shapes_launch_nothing(device):
    from xagents_amd import _lib
    c, _, _ = _case(5, 2, 63, 1.0)
    for N, kappa, msg in ((257, 1.0, 'n_quantiles <= 256'), (63, 0.0, 'huber_kappa')):
        step = torch.full((1,), 41, dtype=torch.int32, device=device)
        with pytest.raises(_lib.HipLibraryError, match=msg):
            _td(device, c, kappa, False, adam_step=step, N=N)
        torch.cuda.synchronize()
        assert int(step.item()) == 41
    theta = _dev(device, c['theta'])
    act = torch.full((5,), -7, dtype=torch.int32, device=device)
    with pytest.raises(_lib.HipLibraryError, match='n_quantiles <= 256'):
        _call('xa_qr_act', theta.data_ptr(), 5, 2, 257, None, 0, act.data_ptr(), None)
    assert (act.cpu().numpy() == -7).all()


# ---- 4. agent --------------------------------------------------------------------------------
MLP_CFG = ('[dense-0]\nunits=32\nactivation=relu\n\n[dense-1]\nunits=16\nactivation=relu\n\n'
           '[dense-2]\noutput=1\n')
NQ = 8


def _qrdqn(device, tmp_path, n=4, cls=None, model_seed=9, **kwargs):
    from xagents_amd import QRDQN
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    np.random.seed(1)
    random.seed(1)
    envs = create_envs('CartPole-v1', n, mode='transitions', device=device, seed=3, t_rec=64)
    cfg = tmp_path / 'ann.cfg'
    cfg.write_text(MLP_CFG)
    model = create_model(envs, 'qrdqn', 'model', seed=model_seed, device=device,
                         model_cfg=str(cfg), optimizer_kwargs=dict(learning_rate=1e-3),
                         n_quantiles=kwargs.pop('model_quantiles', NQ))
    bufs = create_buffers('qrdqn', 16 * n, 2 * n, n, initial_size=8 * n)
    kw = dict(seed=2, quiet=True, epsilon_start=0.0, epsilon_end=0.0, gamma=0.99,
              n_quantiles=NQ)
    kw.update(kwargs)
    return (cls or QRDQN)(envs, model, bufs, **kw)


def _fill(agent):
    """fill_buffers() from one RNG state, so two agents store the same transitions."""
    np.random.seed(7)
    random.seed(7)
    agent.fill_buffers()


def _state(agent):
    opt = agent.model.optimizer
    return [x.cpu().numpy().tobytes() for x in
            (agent.model.theta, agent.target_model.theta, opt.m, opt.v, opt.iterations)]


def _step(agent):
    agent.at_step_start()
    agent.train_step()
    agent.at_step_end()


def _f64_step(agent, th0, tt0, m0, v0, it0, lr=1e-3):
    """(raw gradient, parameters after Keras Adam) of the gathered batch in float64: the
    network oracle's forward / backward around qr_ref's dtheta."""
    import nets_f64 as O
    import oracle as OR
    model = agent.model
    B, A, N = agent.batch_size, agent.n_actions, agent.n_quantiles
    s, s2 = agent.xb[:B].cpu().numpy(), agent.xb[B:].cpu().numpy()
    L, shape, out = model.layers, model.input_shape, model.outputs[0]
    x64, outs = O.forward(L, th0, s, shape)
    next_t = O.forward(L, tt0, s2, shape)[1][out]
    next_o = O.forward(L, th0, s2, shape)[1][out] if agent.double else None
    r = R.td(outs[out], next_t, next_o, agent.b_act.cpu().numpy(), _np(agent.b_rew),
             agent.b_done.cpu().numpy(), 0.99, agent.huber_kappa, A, N)
    r['a_star_target'] = R.greedy(next_t, A, N)
    g = O.backward(L, th0, x64, outs, {out: r['dtheta']})
    th1, _, _ = OR.keras_adam_f64(th0, m0, v0, g, it0 + 1, lr, 0.9, 0.999, 1e-7)
    return g, th1, r


def _train_step_vs_f64(agent):
    agent.fill_buffers()
    # a target net with other greedy actions than the online net's, so double Q matters (a
    # scaled copy of a bias-free ReLU net keeps every argmax): the head's action blocks in
    # reverse order, then the scaling
    A, N = agent.n_actions, agent.n_quantiles
    w = agent.model.get_weights()
    K = w[-2].shape[0]
    w[-2] = np.ascontiguousarray(w[-2].reshape(K, A, N)[:, ::-1]).reshape(K, A * N)
    w[-1] = np.ascontiguousarray(w[-1].reshape(A, N)[::-1]).reshape(A * N)
    agent.target_model.set_weights(w)
    agent.target_model.theta.mul_(0.97)
    model, opt = agent.model, agent.model.optimizer
    th0, tt0 = _np(model.theta), _np(agent.target_model.theta)
    m0, v0, it0 = opt.m.cpu().numpy(), opt.v.cpu().numpy(), int(opt.iterations.item())
    agent.write_raw_grad = True
    _step(agent)
    torch.cuda.synchronize()
    g, th1, r = _f64_step(agent, th0, tt0, m0, v0, it0)
    e = _rel(_np(agent.grad), g)
    print(f'raw gradient rel err {e:.3e}')
    assert np.abs(g).max() > 0 and e < GRAD_TOL
    step_ref, step_got = th1 - th0, model.theta.cpu().numpy() - th0
    # Adam's first step is ~lr * sign(g): compare the update where |g| is not tiny
    big = np.abs(g) > 1e-6 * np.abs(g).max()
    err = np.abs(step_got[big] - step_ref[big]).max() / 1e-3
    assert err < 2e-2, f'Adam step mismatch {err:.3g} (units of lr)'
    assert int(opt.iterations.item()) == it0 + 1 and agent.steps == agent.n_envs
    np.testing.assert_allclose(_np(agent.td_loss), r['loss'], rtol=GRAD_TOL, atol=GRAD_TOL)
    return r


@pytest.mark.parametrize('double', [False, True])
def test_qrdqn_train_step_vs_f64(device, tmp_path, double):
    agent = _qrdqn(device, tmp_path, double=double)
    assert agent.batch_size == 8 and agent.dq.shape == (8, 2 * NQ) and not agent._head_fused()
    r = _train_step_vs_f64(agent)
    if double:  # the online net's a* is not the target net's in every row
        assert (r['a_star'] != r['a_star_target']).any()


def test_qrdqn_nature_cnn_step_vs_f64(device):
    """The wide head on the NatureCNN cfg: the 37632 x 512 layer's Adam runs inside its
    weight-gradient GEMM, the conv stack's inside its backward."""
    from xagents_amd import QRDQN
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    np.random.seed(1)
    random.seed(1)
    envs = create_envs('PongNoFrameskip-v4', 2, device=device, seed=3)
    model = create_model(envs, 'qrdqn', 'model', seed=9, device=device, n_quantiles=4,
                         optimizer_kwargs=dict(learning_rate=1e-3))
    assert model.layers[-1].units == 24
    agent = QRDQN(envs, model, create_buffers('qrdqn', 40, 4, 2, initial_size=20), seed=2,
                  quiet=True, epsilon_start=0.0, epsilon_end=0.0, gamma=0.99, n_quantiles=4)
    assert agent._fused_adam_layers()[0]
    _train_step_vs_f64(agent)


def test_qrdqn_captured_learner_matches_eager(device, tmp_path, monkeypatch):
    out = []
    for use_graph in (False, True):
        monkeypatch.setenv('XA_DQN_LEARN_GRAPH', '1' if use_graph else '0')
        agent = _qrdqn(device, tmp_path, double=True, epsilon_start=1.0,
                       epsilon_decay_steps=8, target_sync_steps=8)
        agent.use_graph = use_graph
        _fill(agent)
        np.random.seed(4)
        random.seed(4)
        for _ in range(3):
            _step(agent)
        torch.cuda.synchronize()
        assert (agent._lgraph is not None) == use_graph
        out.append(_state(agent) + [agent.b_act.cpu().numpy().tobytes(),
                                    agent.dq.cpu().numpy().tobytes()])
    assert out[0] == out[1]


def test_prioritized_qrdqn_with_beta_zero_equals_plain(device, tmp_path):
    per = _qrdqn(device, tmp_path, prioritized=True, per_beta=0.0)
    plain = _qrdqn(device, tmp_path)
    assert per.per is not None and plain.per is None
    for agent in (per, plain):
        _fill(agent)
        agent.target_model.theta.mul_(0.97)
    assert _state(per) == _state(plain)
    for _ in range(2):
        per.train_step()
        torch.cuda.synchronize()
        slots = per.per.slots.cpu().numpy().copy()
        assert (per.per.weights.cpu().numpy() == 1.0).all()
        plain.replay.sample_slots = lambda s=slots: s
        plain.train_step()
        torch.cuda.synchronize()
        assert per.b_act.cpu().numpy().tobytes() == plain.b_act.cpu().numpy().tobytes()
    assert _state(per) == _state(plain)
    assert int(per.model.optimizer.iterations.item()) == 2
    assert int(per.per.counter.item()) == 2  # one draw per gradient step
    assert (per.per.td_abs > 0).all() and torch.isfinite(per.per.td_abs).all()


def test_prioritized_qrdqn_fit_keeps_the_tree(device, tmp_path):
    import per_ref as P
    agent = _qrdqn(device, tmp_path, prioritized=True, per_beta_steps=400, epsilon_start=1.0,
                   epsilon_decay_steps=100)
    agent.fit(max_steps=200)
    torch.cuda.synchronize()
    assert agent.steps >= 200
    assert int(agent.model.optimizer.iterations.item()) == agent.steps // 4
    assert torch.isfinite(agent.td_loss).all() and torch.isfinite(agent.model.theta).all()
    per = agent.per
    leaves = per.leaves.cpu().numpy()
    np.testing.assert_allclose(per.nodes.cpu().numpy(), P.flat(P.build(leaves)), rtol=1e-12,
                               atol=0)
    assert np.count_nonzero(leaves) == int(np.minimum(agent.replay.host_count, 16).sum())
    nodes = per.nodes.cpu().numpy().copy()
    per.rebuild()
    torch.cuda.synchronize()
    assert per.nodes.cpu().numpy().tobytes() == nodes.tobytes()


def test_qrdqn_fit_with_target_syncs(device, tmp_path):
    agent = _qrdqn(device, tmp_path, epsilon_start=1.0, epsilon_decay_steps=200,
                   target_sync_steps=40)
    agent.fit(max_steps=400)
    torch.cuda.synchronize()
    assert agent.steps >= 400
    assert agent.epsilon == pytest.approx(max(0.0, 1.0 - (agent.steps - 4) / 200))
    # 400 % 40 == 0: the target was synced at the last step
    np.testing.assert_array_equal(agent.target_model.theta.cpu().numpy(),
                                  agent.model.theta.cpu().numpy())
    assert int(agent.model.optimizer.iterations.item()) == agent.steps // 4
    assert torch.isfinite(agent.model.theta).all() and len(agent.total_rewards) == agent.games


def test_play_actions_are_the_reference_argmax(device, tmp_path):
    import nets_f64 as O
    agent = _qrdqn(device, tmp_path)
    model = agent.model
    state = agent.envs.state.cpu().numpy()
    theta = O.forward(model.layers, _np(model.theta), state, model.input_shape)[1][
        model.outputs[0]]
    q = R.mean_q(theta, agent.n_actions, NQ)
    assert R.margin(theta, agent.n_actions, NQ) > 1e-5
    act = agent._play_actions()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(act.cpu().numpy(), q.argmax(1))
    np.testing.assert_allclose(_np(agent.q_mean), q, rtol=GRAD_TOL, atol=GRAD_TOL)
    a2, q2 = agent.get_model_outputs(agent.envs.state, agent.model)
    assert a2.cpu().numpy().tobytes() == act.cpu().numpy().tobytes()
    assert q2.cpu().numpy().tobytes() == agent.q_mean.cpu().numpy().tobytes()
    assert agent.play(max_steps=20) >= 0


def test_checkpoint_round_trip_continues_bit_identically(device, tmp_path):
    """Random acting (epsilon 1), so a second agent with other initial weights stores the
    same transitions; after two steps (the second syncs the target) its model loads the
    first's checkpoint and the next step matches bit for bit."""
    kw = dict(epsilon_start=1.0, epsilon_end=1.0, target_sync_steps=8)
    a = _qrdqn(device, tmp_path, **kw)
    b = _qrdqn(device, tmp_path, model_seed=10, **kw)
    assert _state(a) != _state(b)
    for agent in (a, b):
        _fill(agent)
        np.random.seed(5)
        random.seed(5)
        for _ in range(2):
            _step(agent)
    path = tmp_path / 'qrdqn.npz'
    a.model.save_weights(path)
    b.model.load_weights(path)
    b.sync_target_model()  # steps == 8: copies the loaded weights
    torch.cuda.synchronize()
    assert _state(a) == _state(b)
    for agent in (a, b):
        np.random.seed(6)
        random.seed(6)
        _step(agent)
    torch.cuda.synchronize()
    assert _state(a) == _state(b) and int(a.model.optimizer.iterations.item()) == 3


def test_wrong_output_width_raises(device, tmp_path):
    with pytest.raises(AssertionError, match='n_actions \\* n_quantiles'):
        _qrdqn(device, tmp_path, model_quantiles=NQ + 1)
    with pytest.raises(ValueError, match='huber_kappa'):
        _qrdqn(device, tmp_path, huber_kappa=0.0)


def test_overridden_hook_takes_the_composed_path(device, tmp_path):
    from xagents_amd import QRDQN

    class Hooked(QRDQN):
        calls = 0

        def get_targets(self, *batch):
            type(self).calls += 1
            y = super().get_targets(*batch)
            assert y.shape == (self.batch_size, self.n_quantiles)
            return y

    out = []
    for cls in (QRDQN, Hooked):
        agent = _qrdqn(device, tmp_path, cls=cls, double=True)
        _fill(agent)
        agent.target_model.theta.mul_(0.97)
        theta0 = _np(agent.model.theta)
        np.random.seed(8)
        random.seed(8)
        for _ in range(2):
            _step(agent)
        torch.cuda.synchronize()
        out.append((_np(agent.model.theta), agent.b_act.cpu().numpy().copy()))
    assert Hooked.calls == 2
    np.testing.assert_array_equal(out[0][1], out[1][1])
    # the same arithmetic through other launches (torch forms y, the layer executors are
    # rebuilt per call): test_gpu_hooks.py's form, the difference relative to the update
    fused, composed = out[0][0], out[1][0]
    rel = np.linalg.norm(composed - fused) / np.linalg.norm(fused - theta0)
    assert rel < 1e-4, f'composed vs fused update: {rel:.2e}'
