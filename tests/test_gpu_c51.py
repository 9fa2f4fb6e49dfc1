"""GPU tests of categorical DQN (xagents_amd/c51, csrc/c51.hip): the three kernels against the
float64 restatement (tests/c51_ref.py) at its fixed shapes and supports, the composed and the
weighted head bit for bit, and the agent -- train steps against the f64 network oracle seeded
with the restatement's dtheta, the captured learner phase, prioritized replay, n-step batches,
play, checkpoints, the composed path.

Tolerances:
* kernels: c51_ref.bounds, derived there from the arithmetic (no figure is taken from a run);
  the greedy actions are compared exactly (the generator keeps every compared pair of
  expected-Q values 1e-3 and four times the Q limit apart).
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

import c51_ref as R

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / 'oracle'))
pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4
GAMMA = np.float32(R.GAMMA)
CASES = [(*s, *v) for s in R.SHAPES for v in R.SUPPORTS]


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
def _case(B, A, K, v_min, v_max):
    """The fixed inputs and their float64 results (plain / double, gamma / per-row discounts),
    computed once."""
    c = R.case(B, A, K, v_min, v_max)
    ref = {(d, n): R.td(c['theta'], c['next_t'], c['next_o'] if d else None, c['act'],
                        c['rew'], c['done'], R.GAMMA, A, K, v_min, v_max,
                        discounts=c['disc'] if n else None)
           for d in (False, True) for n in (False, True)}
    return c, ref, R.bounds(c)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _project(device, c, double, disc=None, K=None, v=None):
    """xa_c51_project on a case; the output carries a guard row that must stay untouched."""
    B, A = c['B'], c['A']
    v_min, v_max = v or (c['v_min'], c['v_max'])
    t = {k: _dev(device, c[k]) for k in ('next_t', 'next_o', 'rew', 'done')}
    d = None if disc is None else _dev(device, disc)
    m = torch.full((B + 1, c['K']), 7.0, device=device)
    try:
        _call('xa_c51_project', t['next_t'].data_ptr(), _ptr(t['next_o']) if double else None,
              t['rew'].data_ptr(), t['done'].data_ptr(), _ptr(d), B, A, K or c['K'], v_min,
              v_max, float(GAMMA), m.data_ptr())
    finally:
        torch.cuda.synchronize()
        m = m.cpu().numpy()
        assert (m[B] == 7.0).all()
        if K or v:
            assert (m == 7.0).all()
    return m[:B]


def _td(device, c, double, disc=None, weights=None, target_dist=None, K=None, v=None,
        want=('loss', 'td_abs', 'step')):
    """xa_c51_td_grad on a case: dict(dtheta, loss, td_abs); outputs carry a guard row that
    must stay untouched (an illegal K or support: every output untouched)."""
    B, A = c['B'], c['A']
    v_min, v_max = v or (c['v_min'], c['v_max'])
    t = {k: _dev(device, c[k]) for k in ('theta', 'next_t', 'next_o', 'act', 'rew', 'done')}
    extra = [None if x is None else _dev(device, x) for x in (disc, weights, target_dist)]
    d = torch.full((B + 1, A * c['K']), 7.0, device=device)
    loss = torch.full((B + 1,), 7.0, device=device)
    td_abs = torch.full((B + 1,), 7.0, device=device)
    step = torch.full((2,), 41, dtype=torch.int32, device=device)
    given = target_dist is not None
    try:
        _call('xa_c51_td_grad', t['theta'].data_ptr(),
              None if given else t['next_t'].data_ptr(),
              t['next_o'].data_ptr() if double and not given else None, _ptr(extra[2]),
              t['act'].data_ptr(), None if given else t['rew'].data_ptr(),
              None if given else t['done'].data_ptr(), B, A, K or c['K'], v_min, v_max,
              float(GAMMA), d.data_ptr(), loss.data_ptr() if 'loss' in want else None,
              step.data_ptr() if 'step' in want else None, _ptr(extra[1]),
              td_abs.data_ptr() if 'td_abs' in want else None, _ptr(extra[0]))
    finally:
        torch.cuda.synchronize()
        out = dict(dtheta=d.cpu().numpy(), loss=loss.cpu().numpy(), td_abs=td_abs.cpu().numpy())
        bad = bool(K or v)
        for k, x in out.items():
            assert (x[B] == 7.0).all(), k
            if bad or (k != 'dtheta' and k not in want):
                assert (x == 7.0).all(), k
        assert step.cpu().numpy().tolist() == [41 if bad or 'step' not in want else 42, 41]
    return {k: x[:B] for k, x in out.items()}


# ---- 1. kernels against the restatement ---------------------------------------------------
@pytest.mark.parametrize('B,A,K,v_min,v_max', CASES)
def test_c51_act(device, B, A, K, v_min, v_max):
    c, _, bound = _case(B, A, K, v_min, v_max)
    for key in ('theta', 'next_o'):
        logits = _dev(device, c[key])
        act = torch.full((B + 1,), -7, dtype=torch.int32, device=device)
        q = torch.full((B + 1, A), 7.0, device=device)
        _call('xa_c51_act', logits.data_ptr(), B, A, K, v_min, v_max, None, 0, act.data_ptr(),
              q.data_ptr())
        act, q = act.cpu().numpy(), q.cpu().numpy()
        assert act[B] == -7 and (q[B] == 7.0).all()
        np.testing.assert_array_equal(act[:B], R.greedy(c[key], A, K, v_min, v_max))
        err = np.abs(q[:B] - R.expected_q(c[key], A, K, v_min, v_max)).max()
        print(f'Q err {err:.3e} bound {bound["q"]:.3e}')
        assert err <= bound['q']
        # without q_out: the same actions
        act2 = torch.full((B + 1,), -7, dtype=torch.int32, device=device)
        _call('xa_c51_act', logits.data_ptr(), B, A, K, v_min, v_max, None, 0, act2.data_ptr(),
              None)
        np.testing.assert_array_equal(act2.cpu().numpy()[:B], act[:B])
    # use_random copies the given actions (and reads no logits)
    given = _dev(device, np.random.default_rng(B).integers(0, A, B).astype(np.int32))
    out = torch.full((B + 1,), -7, dtype=torch.int32, device=device)
    _call('xa_c51_act', None, B, A, K, v_min, v_max, given.data_ptr(), 1, out.data_ptr(), None)
    out = out.cpu().numpy()
    assert out[B] == -7 and out[:B].tobytes() == given.cpu().numpy().tobytes()


@pytest.mark.parametrize('nstep', [False, True])
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('B,A,K,v_min,v_max', CASES)
def test_c51_project_and_td_grad(device, B, A, K, v_min, v_max, double, nstep):
    c, ref, bound = _case(B, A, K, v_min, v_max)
    want = ref[(double, nstep)]
    disc = c['disc'] if nstep else None
    m = _project(device, c, double, disc)
    got = _td(device, c, double, disc)
    off = np.ones((B, A, K), bool)
    off[np.arange(B), c['act']] = False
    assert (got['dtheta'].reshape(B, A, K)[off] == 0).all()
    e_m = np.abs(m - want['m']).max()
    e_s = np.abs(m.astype(np.float64).sum(1) - 1.0).max()
    e_g = np.abs(got['dtheta'] - want['dtheta']).max()
    e_l = np.abs(got['loss'] - want['loss']).max()
    e_t = np.abs(got['td_abs'] - want['td_abs']).max()
    print(f'm err {e_m:.3e} bound {bound["m"]:.3e}; mass err {e_s:.3e} bound '
          f'{bound["mass"]:.3e}; grad err {e_g:.3e} bound {bound["grad"]:.3e} (x B: '
          f'{e_g * B:.3e}); loss err {e_l:.3e} bound {bound["loss"]:.3e}; '
          f'td_abs err {e_t:.3e} bound {bound["td_abs"]:.3e}')
    assert np.abs(want['dtheta']).max() > 1e-3 / (B * K)
    assert e_m <= bound['m'] and e_s <= bound['mass']
    assert e_g <= bound['grad']
    assert e_l <= bound['loss']
    assert e_t <= bound['td_abs']
    # the composed form: the head given xa_c51_project's m writes the fused call's bytes
    comp = _td(device, c, double, target_dist=m)
    for k in got:
        assert comp[k].tobytes() == got[k].tobytes(), k


# ---- 2. weights and discounts, bit for bit ---------------------------------------------------
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('B,A,K,v_min,v_max', [(5, 2, 51, -10.0, 10.0), (65, 6, 2, 0.0, 200.0),
                                               (5, 6, 256, -1.0, 1.0)])
def test_c51_td_head_weights_and_discounts(device, B, A, K, v_min, v_max, double):
    c, ref, bound = _case(B, A, K, v_min, v_max)
    base = _td(device, c, double)
    again = _td(device, c, double)  # null weights twice: the same bytes
    same = _td(device, c, double, disc=np.full(B, GAMMA, np.float32))  # all-gamma discounts
    for k in base:
        assert again[k].tobytes() == base[k].tobytes() == same[k].tobytes(), k
    m0 = _project(device, c, double)
    assert _project(device, c, double, np.full(B, GAMMA, np.float32)).tobytes() == m0.tobytes()
    w = c['weights']
    wt = _td(device, c, double, weights=w)
    assert wt['dtheta'].tobytes() == (base['dtheta'] * w[:, None]).tobytes()
    assert wt['loss'].tobytes() == (base['loss'] * w).tobytes()
    # td_abs is not weighted, and asking for fewer outputs changes nothing else
    assert wt['td_abs'].tobytes() == base['td_abs'].tobytes()
    bare = _td(device, c, double, want=())
    assert bare['dtheta'].tobytes() == base['dtheta'].tobytes()


# ---- 3. illegal shapes and supports ----------------------------------------------------------
def test_illegal_shapes_and_supports_launch_nothing(device):
    from xagents_amd import _lib
    c, _, _ = _case(5, 2, 51, -10.0, 10.0)
    bad = [(dict(K=257), 'n_atoms <= 256'), (dict(K=1), '2 <= n_atoms'),
           (dict(v=(1.0, 1.0)), 'v_max > v_min'), (dict(v=(10.0, -10.0)), 'v_max > v_min'),
           (dict(v=(-10.0, float('inf'))), 'v_max > v_min'),
           (dict(v=(float('nan'), 10.0)), 'v_max > v_min')]
    for kw, msg in bad:
        with pytest.raises(_lib.HipLibraryError, match=msg):
            _td(device, c, False, **kw)  # (asserts every output untouched)
        with pytest.raises(_lib.HipLibraryError, match=msg):
            _project(device, c, False, **kw)
        logits = _dev(device, c['theta'])
        act = torch.full((5,), -7, dtype=torch.int32, device=device)
        q = torch.full((5, 2), 7.0, device=device)
        v_min, v_max = kw.get('v', (-10.0, 10.0))
        with pytest.raises(_lib.HipLibraryError, match=msg):
            _call('xa_c51_act', logits.data_ptr(), 5, 2, kw.get('K', 51), v_min, v_max, None, 0,
                  act.data_ptr(), q.data_ptr())
        torch.cuda.synchronize()
        assert (act.cpu().numpy() == -7).all() and (q.cpu().numpy() == 7.0).all()


# ---- 4. agent --------------------------------------------------------------------------------
MLP_CFG = ('[dense-0]\nunits=32\nactivation=relu\n\n[dense-1]\nunits=16\nactivation=relu\n\n'
           '[dense-2]\noutput=1\n')
NA = 8
SUPPORT = dict(v_min=-2.0, v_max=12.0)  # CartPole rewards are 1: targets inside and clipped


def _c51(device, tmp_path, n=4, cls=None, model_seed=9, **kwargs):
    from xagents_amd import C51
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    np.random.seed(1)
    random.seed(1)
    envs = create_envs('CartPole-v1', n, mode='transitions', device=device, seed=3, t_rec=64)
    cfg = tmp_path / 'ann.cfg'
    cfg.write_text(MLP_CFG)
    model = create_model(envs, 'c51', 'model', seed=model_seed, device=device,
                         model_cfg=str(cfg), optimizer_kwargs=dict(learning_rate=1e-3),
                         n_atoms=kwargs.pop('model_atoms', NA))
    bufs = create_buffers('c51', 16 * n, 2 * n, n, initial_size=8 * n)
    kw = dict(seed=2, quiet=True, epsilon_start=0.0, epsilon_end=0.0, gamma=0.99, n_atoms=NA,
              **SUPPORT)
    kw.update(kwargs)
    return (cls or C51)(envs, model, bufs, **kw)


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


def _reverse_target_actions(agent):
    """A target net with other greedy actions than the online net's, so double Q matters: the
    head's action blocks in reverse order, then a scaling."""
    A, K = agent.n_actions, agent.n_atoms
    w = agent.model.get_weights()
    H = w[-2].shape[0]
    w[-2] = np.ascontiguousarray(w[-2].reshape(H, A, K)[:, ::-1]).reshape(H, A * K)
    w[-1] = np.ascontiguousarray(w[-1].reshape(A, K)[::-1]).reshape(A * K)
    agent.target_model.set_weights(w)
    agent.target_model.theta.mul_(0.97)


def _f64_head(agent, th0, tt0, rew, disc, weights=None):
    """(raw gradient, c51_ref.td's dict) of the gathered batch in float64: the network oracle's
    forward / backward around c51_ref's dtheta."""
    import nets_f64 as O
    model = agent.model
    B, A, K = agent.batch_size, agent.n_actions, agent.n_atoms
    s, s2 = agent.xb[:B].cpu().numpy(), agent.xb[B:].cpu().numpy()
    L, shape, out = model.layers, model.input_shape, model.outputs[0]
    x64, outs = O.forward(L, th0, s, shape)
    next_t = O.forward(L, tt0, s2, shape)[1][out]
    next_o = O.forward(L, th0, s2, shape)[1][out] if agent.double else None
    r = R.td(outs[out], next_t, next_o, agent.b_act.cpu().numpy(), rew,
             agent.b_done.cpu().numpy(), 0.99, A, K, agent.v_min, agent.v_max, weights, disc)
    r['a_star_target'] = R.greedy(next_t, A, K, agent.v_min, agent.v_max)
    return O.backward(L, th0, x64, outs, {out: r['dtheta']}), r


def _train_steps_vs_f64(agent, steps=3):
    import oracle as OR
    agent.fill_buffers()
    _reverse_target_actions(agent)
    model, opt = agent.model, agent.model.optimizer
    agent.write_raw_grad = True
    differs = False
    for k in range(steps):
        th0, tt0 = _np(model.theta), _np(agent.target_model.theta)
        m0, v0, it0 = opt.m.cpu().numpy(), opt.v.cpu().numpy(), int(opt.iterations.item())
        agent.at_step_start()
        agent.train_step()
        torch.cuda.synchronize()
        g, r = _f64_head(agent, th0, tt0, _np(agent.b_rew), None)
        e = _rel(_np(agent.grad), g)
        print(f'step {k}: raw gradient rel err {e:.3e}')
        assert np.abs(g).max() > 0 and e < GRAD_TOL
        th1, _, _ = OR.keras_adam_f64(th0, m0, v0, g, it0 + 1, 1e-3, 0.9, 0.999, 1e-7)
        step_ref, step_got = th1 - th0, model.theta.cpu().numpy() - th0
        if k == 0:
            # Adam's first step is ~lr * sign(g): compare the update where |g| is not tiny
            big = np.abs(g) > 1e-6 * np.abs(g).max()
            err = np.abs(step_got[big] - step_ref[big]).max() / 1e-3
            assert err < 2e-2, f'Adam step mismatch {err:.3g} (units of lr)'
        assert int(opt.iterations.item()) == it0 + 1
        np.testing.assert_allclose(_np(agent.td_loss), r['loss'], rtol=GRAD_TOL, atol=GRAD_TOL)
        differs |= bool((r['a_star'] != r['a_star_target']).any())
        agent.at_step_end()
    assert agent.steps == steps * agent.n_envs
    return differs


@pytest.mark.parametrize('double', [False, True])
def test_c51_train_steps_vs_f64(device, tmp_path, double):
    agent = _c51(device, tmp_path, double=double)
    assert agent.batch_size == 8 and agent.dq.shape == (8, 2 * NA) and not agent._head_fused()
    differs = _train_steps_vs_f64(agent)
    assert differs == double  # the online net's a* is not the target net's in every row


@pytest.mark.parametrize('double', [False, True])
def test_c51_nature_cnn_steps_vs_f64(device, double):
    """The wide head on the NatureCNN cfg: the 37632 x 512 layer's Adam runs inside its
    weight-gradient GEMM, the conv stack's inside its backward."""
    from xagents_amd import C51
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    np.random.seed(1)
    random.seed(1)
    envs = create_envs('PongNoFrameskip-v4', 2, device=device, seed=3)
    model = create_model(envs, 'c51', 'model', seed=9, device=device, n_atoms=4,
                         optimizer_kwargs=dict(learning_rate=1e-3))
    assert model.layers[-1].units == 24
    agent = C51(envs, model, create_buffers('c51', 40, 4, 2, initial_size=20), seed=2,
                quiet=True, epsilon_start=0.0, epsilon_end=0.0, gamma=0.99, n_atoms=4,
                double=double, v_min=-1.0, v_max=1.0)
    assert agent._fused_adam_layers()[0]
    _train_steps_vs_f64(agent)


def test_c51_captured_learner_matches_eager(device, tmp_path, monkeypatch):
    out = []
    for use_graph in (False, True):
        monkeypatch.setenv('XA_DQN_LEARN_GRAPH', '1' if use_graph else '0')
        agent = _c51(device, tmp_path, double=True, epsilon_start=1.0, epsilon_decay_steps=8,
                     target_sync_steps=8)
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


def test_prioritized_c51_with_beta_zero_equals_plain(device, tmp_path):
    per = _c51(device, tmp_path, prioritized=True, per_beta=0.0)
    plain = _c51(device, tmp_path)
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


def test_c51_trains_on_the_n_step_batch(device, tmp_path):
    """Three train steps with n_steps = 3: the gathered batch is nstep_ref's restatement
    applied to the rings at the slots the step used, and the raw gradient follows from it."""
    import nstep_ref as NS
    agent = _c51(device, tmp_path, n_steps=3, double=True)
    assert agent.n_steps == 3 and agent.b_disc.shape == (8,)
    _fill(agent)
    _reverse_target_actions(agent)
    agent.write_raw_grad = True
    B = agent.batch_size
    seen_m = set()
    for _ in range(3):
        th0, tt0 = _np(agent.model.theta), _np(agent.target_model.theta)
        agent.at_step_start()
        agent.train_step()
        torch.cuda.synchronize()
        rp = agent.replay
        rings = dict(states=rp.states.cpu().numpy(), new_states=rp.new_states.cpu().numpy(),
                     actions=rp.actions.cpu().numpy(), rewards=rp.rewards.cpu().numpy(),
                     dones=rp.dones.cpu().numpy())
        count = rp.count.cpu().numpy()
        slots = agent._gather_stage().host(0).numpy().copy()
        want = NS.gather(rings, count, slots, 3, GAMMA, np.float32)
        got = dict(states=agent.xb[:B], new_states=agent.xb[B:], actions=agent.b_act,
                   rewards=agent.b_rew, dones=agent.b_done, discounts=agent.b_disc)
        for k, v in got.items():
            assert v.cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
        seen_m |= set((want['L'] + 1).tolist())
        ref64 = NS.gather(rings, count, slots, 3, GAMMA, np.float64)
        g, r = _f64_head(agent, th0, tt0, ref64['rewards'], ref64['discounts'])
        e = _rel(_np(agent.grad), g)
        print(f'raw gradient rel err {e:.3e}')
        assert np.abs(g).max() > 0 and e < GRAD_TOL
        np.testing.assert_allclose(_np(agent.td_loss), r['loss'], rtol=GRAD_TOL, atol=GRAD_TOL)
        agent.at_step_end()
    assert 3 in seen_m  # (some sampled slot had three steps ahead of it)
    assert int(agent.model.optimizer.iterations.item()) == 3


def test_play_actions_are_the_reference_argmax(device, tmp_path):
    import nets_f64 as O
    agent = _c51(device, tmp_path)
    model = agent.model
    state = agent.envs.state.cpu().numpy()
    logits = O.forward(model.layers, _np(model.theta), state, model.input_shape)[1][
        model.outputs[0]]
    sup = (agent.n_actions, NA, agent.v_min, agent.v_max)
    q = R.expected_q(logits, *sup)
    assert R.margin(logits, *sup) > 1e-4
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
    a = _c51(device, tmp_path, **kw)
    b = _c51(device, tmp_path, model_seed=10, **kw)
    assert _state(a) != _state(b)
    for agent in (a, b):
        _fill(agent)
        np.random.seed(5)
        random.seed(5)
        for _ in range(2):
            _step(agent)
    path = tmp_path / 'c51.npz'
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
    with pytest.raises(AssertionError, match='n_actions \\* n_atoms'):
        _c51(device, tmp_path, model_atoms=NA + 1)


def test_overridden_hook_takes_the_composed_path(device, tmp_path):
    from xagents_amd import C51

    class Hooked(C51):
        calls = 0

        def get_targets(self, *batch):
            type(self).calls += 1
            m = super().get_targets(*batch)
            assert m.shape == (self.batch_size, self.n_atoms)
            return m

    out = []
    for cls in (C51, Hooked):
        agent = _c51(device, tmp_path, cls=cls, double=True)
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
    # the same head arithmetic through other launches (the layer executors are rebuilt per
    # call): test_gpu_hooks.py's form, the difference relative to the update
    fused, composed = out[0][0], out[1][0]
    rel = np.linalg.norm(composed - fused) / np.linalg.norm(fused - theta0)
    assert rel < 1e-4, f'composed vs fused update: {rel:.2e}'
    hooked = _c51(device, tmp_path, cls=Hooked, n_steps=2)
    _fill(hooked)
    with pytest.raises(NotImplementedError, match='discounts'):
        hooked.train_step()
