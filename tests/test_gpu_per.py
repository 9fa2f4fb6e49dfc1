"""GPU tests of prioritized replay (xagents_amd/per.py, csrc/per.hip, the weighted TD heads):
the 64-ary sum tree against the float64 restatement (tests/per_ref.py) built from the device's
own leaves, the sampler's slots exactly (every compared sample keeps a margin of 1e-9 of the
root from the nearest boundary at which the choice changes), the mark rule on wrapping rings of
both kinds, the weighted heads bit for bit, and prioritized DQN / SAC agents against plain ones
and against the f64 oracle's per-sample gradients.

Tolerances:
* nodes: 1e-12 relative. A node is an f64 sum of <= 64 non-negative terms; the device's
  pairwise order and numpy's differ by a few ulps (2.2e-16 each).
* leaves written by xa_per_update: 1e-5 relative. f32 powf as exp(alpha log x) amplifies its
  ulps by |alpha ln x| + 2, <= ~10 for the priorities used here: ~1e-6.
* weights: 1e-6 relative. f64 arithmetic rounded once to f32 (6e-8), on a root that differs
  from the reference's by f64 rounding.
* raw gradients through the layer executor: the project's 1e-4 relative (tests/test_gpu_scale.py).
"""
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import per_ref as R

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / 'oracle'))
pytestmark = pytest.mark.gpu

MARGIN = 1e-9
NODE_RTOL = 1e-12
LEAF_RTOL = 1e-5
WEIGHT_RTOL = 1e-6
GRAD_TOL = 1e-4
ALPHA, EPS = 0.6, 1e-6


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.linalg.norm(np.asarray(got, np.float64) - want) /
                 max(np.linalg.norm(want), 1e-30))


def _dev(device, x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(device)


class _Rings:
    """The part of DeviceReplay the sampler reads: n rings of cap rows, the device counters
    and their host mirror."""

    def __init__(self, device, n, cap, count=None, k=1):
        self.n, self.cap, self.k, self.device = n, cap, k, device
        self.set_count(np.full(n, cap, np.int64) if count is None else count)

    def set_count(self, count):
        self.host_count = np.asarray(count, np.int64)
        self.count = torch.from_numpy(self.host_count.copy()).to(self.device)


def _sampler(device, n, cap, B, leaves=None, beta=0.4, count=None, seed=5):
    from xagents_amd.per import PrioritizedSampler
    s = PrioritizedSampler(_Rings(device, n, cap, count), ALPHA, beta, EPS, seed, batch=B)
    if leaves is not None:
        s.leaves.copy_(_dev(device, leaves))
        s.rebuild()
    return s


def _check_tree(s):
    """Every node against the reference built from the device's own leaves."""
    torch.cuda.synchronize()
    leaves = s.leaves.cpu().numpy()
    want = R.flat(R.build(leaves))
    got = s.nodes.cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=NODE_RTOL, atol=0)
    return leaves, want[-1]


def _stored_td(slots, td):
    """The TD error each item's slot keeps: of the items that list one slot, the last one's."""
    last = {int(slot): b for b, slot in enumerate(slots)}
    return np.asarray(td)[[last[int(slot)] for slot in slots]]


# ---- 1. rebuild and update ------------------------------------------------------------------
@pytest.mark.parametrize('B', R.BATCHES)
@pytest.mark.parametrize('n,cap', R.SHAPES)
def test_rebuild_and_update(device, n, cap, B):
    L = n * cap
    s = _sampler(device, n, cap, B, R.case_leaves(n, cap))
    before, _ = _check_tree(s)
    assert (before == 0).sum() > L // 4 and (before > 0).sum() > L // 4
    # a batch with a repeated slot (its last item's TD error is the one stored), two slots
    # under one level-1 node and, where the tree has more than one, slots under different
    # level-1 nodes
    rng = np.random.default_rng(L + B)
    slots = rng.integers(0, L, B)
    slots[0] = (L // 2) & ~1
    if B >= 2:
        slots[1] = slots[0]
    if B >= 3:
        slots[2] = slots[0] + 1
        assert slots[2] // 64 == slots[0] // 64
    if B >= 4 and L > 64:
        slots[3] = L - 1  # the ragged last node's last leaf
        assert slots[3] // 64 != slots[0] // 64
    td_of_item = rng.uniform(0.0, 0.9, B).astype(np.float32)
    td_of_item[-1] = 0.0  # a zero TD error keeps the priority eps
    mp = 1.0
    for scale in (1.0, 3.0):  # the first batch stays under max_priority = 1, the second not
        td = (td_of_item * np.float32(scale)).astype(np.float32)
        s.slots.copy_(torch.from_numpy(slots).to(device))
        s.td_abs.copy_(_dev(device, td))
        s.update()
        after, _ = _check_tree(s)
        want = (_stored_td(slots, td).astype(np.float64) + EPS) ** ALPHA
        np.testing.assert_allclose(after[slots], want, rtol=LEAF_RTOL, atol=0)
        untouched = np.ones(L, bool)
        untouched[slots] = False
        assert after[untouched].tobytes() == before[untouched].tobytes()
        mp = max(np.float32(mp), (td + np.float32(EPS)).max())
        assert s.max_priority.item() == mp
        before = after
    assert B == 1 or mp > 1.0


# ---- 2. sample --------------------------------------------------------------------------------
@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('B', R.BATCHES)
@pytest.mark.parametrize('n,cap', R.SHAPES)
def test_sample_with_given_uniforms(device, n, cap, B, flip):
    """u = 0 and u = 1 - 2^-24 in the first and the last stratum (and flipped): the slots are
    the reference's on the device's leaves, exactly; leaf_p the leaves; the weights the
    batch-max form."""
    s = _sampler(device, n, cap, B, R.case_leaves(n, cap))
    leaves, root = _check_tree(s)
    u = R.case_uniforms(n, cap, B, flip)
    u_out = torch.full((B,), 7.0, device=device)
    c0 = int(s.counter.item())
    s.sample(u_in=_dev(device, u), u_out=u_out)
    torch.cuda.synchronize()
    assert int(s.counter.item()) == c0  # given uniforms draw nothing
    want, margin = R.sample(leaves, u)
    assert margin.min() >= MARGIN
    slots = s.slots.cpu().numpy()
    np.testing.assert_array_equal(slots, want)
    assert u_out.cpu().numpy().tobytes() == u.tobytes()
    leaf_p = s.leaf_p.cpu().numpy()
    assert leaf_p.tobytes() == leaves[slots].tobytes() and (leaf_p > 0).all()
    w = R.weights(leaf_p, root, R.stored(s.replay.host_count, cap), np.float32(0.4))
    got = s.weights.cpu().numpy()
    np.testing.assert_allclose(got, w, rtol=WEIGHT_RTOL, atol=0)
    assert got.max() == 1.0


@pytest.mark.parametrize('B', R.BATCHES)
@pytest.mark.parametrize('n,cap', R.SHAPES)
def test_sample_philox_path(device, n, cap, B):
    """u_out fed back as u_in gives identical slots; the same counter repeats; another
    counter draws other uniforms (and sample() bumps the counter once)."""
    s = _sampler(device, n, cap, B, R.case_leaves(n, cap))
    s.counter.fill_(5)
    u1 = torch.full((B,), 7.0, device=device)
    s.sample(u_out=u1)
    torch.cuda.synchronize()
    assert int(s.counter.item()) == 6
    slots1, w1 = s.slots.cpu().numpy().copy(), s.weights.cpu().numpy().copy()
    u = u1.cpu().numpy()
    assert (u >= 0).all() and (u < 1).all() and (u * 2.0 ** 24 == np.round(u * 2.0 ** 24)).all()
    s.sample(u_in=u1)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(s.slots.cpu().numpy(), slots1)
    assert s.weights.cpu().numpy().tobytes() == w1.tobytes()
    u2 = torch.full((B,), 7.0, device=device)
    s.sample(u_out=u2)  # counter 6
    torch.cuda.synchronize()
    assert int(s.counter.item()) == 7 and not np.array_equal(u2.cpu().numpy(), u)
    s.counter.fill_(5)
    u3 = torch.full((B,), 7.0, device=device)
    s.sample(u_out=u3)
    torch.cuda.synchronize()
    assert u3.cpu().numpy().tobytes() == u.tobytes()
    np.testing.assert_array_equal(s.slots.cpu().numpy(), slots1)
    # the reference finds the same leaves from the uniforms the device drew (where no draw
    # sits within the margin of a boundary)
    want, margin = R.sample(s.leaves.cpu().numpy(), u)
    ok = margin >= MARGIN
    np.testing.assert_array_equal(slots1[ok], want[ok])


def test_partial_rings_never_return_a_zero_leaf(device):
    """Some envs empty, some partly filled, some wrapped: only written rows are returned, and
    N = sum min(count, cap) is the device's own sum (the weights agree with it)."""
    n, cap, B = 17, 241, 256
    rng = np.random.default_rng(9)
    count = rng.integers(0, 2 * cap, n)
    count[[0, 5, 16]] = 0
    count[3] = 1
    leaves = np.zeros((n, cap), np.float32)
    for e in range(n):
        rows = min(count[e], cap)
        leaves[e, :rows] = rng.uniform(0.01, 2.0, rows)
    s = _sampler(device, n, cap, B, leaves.ravel(), count=count)
    flat, root = _check_tree(s)
    for c in range(4):
        s.counter.fill_(c)
        s.sample()
        torch.cuda.synchronize()
        slots = s.slots.cpu().numpy()
        assert (flat[slots] > 0).all()
        assert (slots % cap < np.minimum(count, cap)[slots // cap]).all()
        w = R.weights(s.leaf_p.cpu().numpy(), root, R.stored(count, cap), np.float32(0.4))
        np.testing.assert_allclose(s.weights.cpu().numpy(), w, rtol=WEIGHT_RTOL, atol=0)


@pytest.mark.parametrize('n,cap', R.SHAPES)
def test_beta_zero_gives_unit_weights(device, n, cap):
    s = _sampler(device, n, cap, 256, R.case_leaves(n, cap), beta=0.0)
    s.sample()
    torch.cuda.synchronize()
    assert (s.weights.cpu().numpy() == 1.0).all()
    s.set_beta(1.0)  # beta is read on device: w leaf is constant over the batch
    s.sample()
    torch.cuda.synchronize()
    wl = _np(s.weights) * _np(s.leaf_p)
    np.testing.assert_allclose(wl, wl[0], rtol=2 * WEIGHT_RTOL)


def test_sample_from_empty_rings_raises(device):
    s = _sampler(device, 2, 35, 7, count=np.zeros(2, np.int64))
    with pytest.raises(ValueError, match='empty'):
        s.sample()


# ---- 3. mark ----------------------------------------------------------------------------------
MLP_CFG = ('[dense-0]\nunits=32\nactivation=relu\n\n[dense-1]\nunits=16\nactivation=relu\n\n'
           '[dense-2]\noutput=1\n')


def _dqn(device, tmp_path, n=4, bufs=None, **kwargs):
    from xagents_amd import DQN
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    np.random.seed(1)
    random.seed(1)
    envs = create_envs('CartPole-v1', n, mode='transitions', device=device, seed=3, t_rec=64)
    cfg = tmp_path / 'ann.cfg'
    cfg.write_text(MLP_CFG)
    model = create_model(envs, 'dqn', 'model', seed=9, device=device, model_cfg=str(cfg),
                         optimizer_kwargs=dict(learning_rate=1e-3))
    bufs = bufs or create_buffers('dqn', 16 * n, 2 * n, n, initial_size=8 * n)
    kw = dict(seed=2, quiet=True, epsilon_start=0.0, epsilon_end=0.0, gamma=0.99)
    kw.update(kwargs)
    return DQN(envs, model, bufs, **kw)


@pytest.mark.parametrize('kind', ['rb1', 'rb2'])
def test_mark_follows_the_rings(device, tmp_path, kind):
    """n_envs = 3, cap = 5, 12 steps (the rings wrap; ReplayBuffer2 then overwrites row 0):
    after every step the non-zero leaves are the slots the host mirror says were written, the
    newest leaf is max_priority^alpha and the tree equals a rebuild."""
    from xagents_amd.utils.buffers import ReplayBuffer1, ReplayBuffer2
    n, cap = 3, 5
    bufs = [ReplayBuffer1(cap, batch_size=2) if kind == 'rb1' else
            ReplayBuffer2(cap, 5, batch_size=2) for _ in range(n)]
    agent = _dqn(device, tmp_path, n=n, bufs=bufs, prioritized=True)
    per, replay = agent.per, agent.replay
    assert per.n_leaves == n * cap and float(per.max_priority.item()) == 1.0
    rng = np.random.default_rng(0)
    written = np.zeros(n * cap, bool)
    for t in range(12):
        if t == 6:
            per.max_priority.fill_(2.0)
        newest = R.mark_slots(replay.host_count, cap)
        agent._env_step(torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).to(device))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(replay.count.cpu().numpy(), replay.host_count)
        written[newest] = True
        leaves = per.leaves.cpu().numpy()
        np.testing.assert_array_equal(leaves != 0, written)
        rows = np.minimum(replay.host_count, cap)
        assert written.reshape(n, cap).sum(1).tolist() == rows.tolist()
        # powf within a few ulps of max_priority^alpha (exactly 1 while max_priority is 1)
        mp = 1.0 if t < 6 else 2.0
        np.testing.assert_allclose(leaves[newest], mp ** ALPHA, rtol=4 * 2.0 ** -23, atol=0)
        nodes = per.nodes.cpu().numpy().copy()
        _check_tree(per)
        per.rebuild()
        torch.cuda.synchronize()
        assert per.nodes.cpu().numpy().tobytes() == nodes.tobytes()
    assert (replay.host_count > cap).all() if kind == 'rb1' else (replay.host_count == cap).all()
    assert written.all()


# ---- 4. heads ---------------------------------------------------------------------------------
def _call(name, *args):
    from xagents_amd._lib import call, stream
    call(name, *args, stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize('B', [1, 100])
@pytest.mark.parametrize('A', [2, 6])
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('huber', [0.0, 0.5])
def test_dqn_td_head_weights(device, huber, double, A, B):
    rng = np.random.default_rng(1000 * B + 10 * A + double)
    q, qt, qo = (rng.normal(size=(B, A)).astype(np.float32) for _ in range(3))
    act = rng.integers(0, A, B).astype(np.int32)
    rew = rng.normal(size=B).astype(np.float32)
    done = (rng.random(B) < 0.3).astype(np.float32)
    w = rng.uniform(0.05, 1.0, B).astype(np.float32)
    gamma = np.float32(0.99)
    t = {k: _dev(device, v, v.dtype) for k, v in dict(q=q, qt=qt, qo=qo, act=act, rew=rew,
                                                       done=done, w=w).items()}

    def run(name, *extra):
        dq = torch.full((B + 1, A), 7.0, device=device)
        loss = torch.full((B + 1,), 7.0, device=device)
        _call(name, t['q'].data_ptr(), t['qt'].data_ptr(),
              t['qo'].data_ptr() if double else None, t['act'].data_ptr(), t['rew'].data_ptr(),
              t['done'].data_ptr(), B, A, float(gamma), huber, dq.data_ptr(), loss.data_ptr(),
              None, *extra)
        dq, loss = dq.cpu().numpy(), loss.cpu().numpy()
        assert (dq[B] == 7.0).all() and loss[B] == 7.0
        return dq[:B], loss[:B]

    dq0, loss0 = run('xa_dqn_td_grad')
    dq1, loss1 = run('xa_dqn_td_grad_w', None, None)
    assert dq1.tobytes() == dq0.tobytes() and loss1.tobytes() == loss0.tobytes()
    td_abs = torch.full((B + 1,), 7.0, device=device)
    dq2, loss2 = run('xa_dqn_td_grad_w', t['w'].data_ptr(), td_abs.data_ptr())
    assert dq2.tobytes() == (dq0 * w[:, None]).tobytes()
    assert loss2.tobytes() == (loss0 * w).tobytes()
    # |y - Q[a]| in f32 from the same inputs, operation by operation (td_terms.hpp)
    rows = np.arange(B)
    v = qt[rows, qo.argmax(1)] if double else qt.max(1)
    v = np.where(done != 0, np.float32(0), v)
    y = v * gamma + rew
    want = np.abs(y - q[rows, act])
    assert want.dtype == np.float32
    got = td_abs.cpu().numpy()
    assert got[B] == 7.0 and got[:B].tobytes() == want.tobytes()
    if huber:
        assert B == 1 or (want > huber).any()  # unclipped beyond delta


@pytest.mark.parametrize('B', [1, 100])
@pytest.mark.parametrize('huber', [0.0, 0.5])
def test_sac_td_head_weights(device, huber, B):
    """log_alpha = 0, where xa_expf returns exactly 1, so the soft target is a plain f32
    expression of the inputs."""
    rng = np.random.default_rng(B)
    v1, v2, tv1, tv2, rew = (rng.normal(size=B).astype(np.float32) for _ in range(5))
    logp = (2 * rng.normal(size=B)).astype(np.float32)
    done = (rng.random(B) < 0.3).astype(np.float32)
    w = rng.uniform(0.05, 1.0, B).astype(np.float32)
    gamma = np.float32(0.99)
    la = np.zeros(1, np.float32)
    t = [_dev(device, x) for x in (v1, v2, tv1, tv2, logp, la, rew, done)]
    tw = _dev(device, w)

    def run(name, *extra):
        out = [torch.full((B + 1,), 7.0, device=device) for _ in range(3)]
        _call(name, *(x.data_ptr() for x in t), B, float(gamma), huber,
              *(o.data_ptr() for o in out), *extra)
        out = [o.cpu().numpy() for o in out]
        assert all(o[B] == 7.0 for o in out)
        return [o[:B] for o in out]

    base = run('xa_sac_td_grad')
    same = run('xa_sac_td_grad_w', None, None)
    for a, b in zip(base, same):
        assert a.tobytes() == b.tobytes()
    td_abs = torch.full((B + 1,), 7.0, device=device)
    dv1, dv2, loss = run('xa_sac_td_grad_w', tw.data_ptr(), td_abs.data_ptr())
    assert dv1.tobytes() == (base[0] * w).tobytes()
    assert dv2.tobytes() == (base[1] * w).tobytes()
    assert loss.tobytes() == (base[2] * w).tobytes()
    soft = np.minimum(tv1, tv2) - np.float32(1.0) * logp
    y = rew + ((np.float32(1.0) - done) * gamma) * soft
    want = np.float32(0.5) * (np.abs(v1 - y) + np.abs(v2 - y))
    assert want.dtype == np.float32
    got = td_abs.cpu().numpy()
    assert got[B] == 7.0 and got[:B].tobytes() == want.tobytes()


# ---- 5. agents --------------------------------------------------------------------------------
def _fill(agent):
    """fill_buffers() from one RNG state, so two agents store the same transitions."""
    np.random.seed(7)
    random.seed(7)
    agent.fill_buffers()


def _spread_priorities(per):
    """Distinct priorities on the stored slots (a loaded leaf array, then a rebuild), so the
    importance weights differ from the first batch on."""
    leaves = per.leaves.cpu().numpy()
    rng = np.random.default_rng(3)
    leaves = (leaves * rng.uniform(0.2, 1.0, len(leaves))).astype(np.float32)
    per.leaves.copy_(torch.from_numpy(leaves).to(per.leaves.device))
    per.rebuild()


def _dqn_state(agent):
    opt = agent.model.optimizer
    return [x.cpu().numpy().tobytes() for x in
            (agent.model.theta, agent.target_model.theta, opt.m, opt.v, opt.iterations)]


@pytest.mark.parametrize('double', [False, True])
def test_prioritized_dqn_with_beta_zero_equals_plain(device, tmp_path, double):
    """beta = 0 (all weights 1), constant over the run: a plain agent fed the prioritized
    agent's slots has the same parameters after 3 chained gradient steps, bit for bit."""
    per = _dqn(device, tmp_path, double=double, prioritized=True, per_beta=0.0)
    plain = _dqn(device, tmp_path, double=double)
    assert per.per is not None and plain.per is None and per.batch_size == 8
    for agent in (per, plain):
        _fill(agent)
        agent.target_model.theta.mul_(0.97)
    assert _dqn_state(per) == _dqn_state(plain)
    assert per.replay.actions.cpu().numpy().tobytes() == plain.replay.actions.cpu().numpy().tobytes()
    for _ in range(3):
        per.train_step()
        torch.cuda.synchronize()
        slots = per.per.slots.cpu().numpy().copy()  # copied back once per step
        assert (per.per.weights.cpu().numpy() == 1.0).all()
        plain.replay.sample_slots = lambda s=slots: s
        plain.train_step()
        torch.cuda.synchronize()
        assert per.b_act.cpu().numpy().tobytes() == plain.b_act.cpu().numpy().tobytes()
    assert _dqn_state(per) == _dqn_state(plain)
    assert int(per.model.optimizer.iterations.item()) == 3
    assert int(per.per.counter.item()) == 3  # one bump per gradient step
    batch = per.concat_buffer_samples()
    assert len(batch) == 5 and batch[0].shape[0] == 8 and int(per.per.counter.item()) == 4


def _dqn_per_sample_f64(agent, th, tt):
    """(|TD error| [B], per-sample gradients [B, P]) of the gathered batch in float64."""
    import nets_f64 as O
    model = agent.model
    B = agent.batch_size
    s, s2 = agent.xb[:B].cpu().numpy(), agent.xb[B:].cpu().numpy()
    a = agent.b_act.cpu().numpy()
    r, d = _np(agent.b_rew), agent.b_done.cpu().numpy()
    L, shape, out = model.layers, model.input_shape, model.outputs[0]
    x64, outs = O.forward(L, th, s, shape)
    q = outs[out]
    qt = O.forward(L, tt, s2, shape)[1][out]
    v = np.where(d != 0, 0.0, qt.max(1))
    y = v * np.float64(np.float32(0.99)) + r
    diff = y - q[np.arange(B), a]
    grads = []
    for b in range(B):
        dq = np.zeros_like(q)
        dq[b, a[b]] = -2.0 * diff[b] / q.shape[1]
        grads.append(O.backward(L, th, x64, outs, {out: dq}))
    return np.abs(diff), np.stack(grads)


def test_prioritized_dqn_gradient_vs_f64(device, tmp_path):
    """beta = 0.4: each step's raw gradient is the f64 per-sample gradients of the same batch
    combined with the device's weights; the sampled leaves afterwards are
    (td_abs + eps)^alpha (a slot sampled twice keeps its last item's)."""
    agent = _dqn(device, tmp_path, prioritized=True, per_beta=0.4)
    _fill(agent)
    agent.target_model.theta.mul_(0.97)
    per = agent.per
    _spread_priorities(per)
    for k in range(3):
        th, tt = _np(agent.model.theta), _np(agent.target_model.theta)
        agent.train_step()
        torch.cuda.synchronize()
        w = _np(per.weights)
        assert w.max() == 1.0 and (w > 0).all() and w.min() < 1.0
        td64, g64 = _dqn_per_sample_f64(agent, th, tt)
        e = _rel(_np(agent.grad), (w[:, None] * g64).sum(0))
        assert e < GRAD_TOL, f'step {k}: raw gradient {e:.2e}'
        td = _np(per.td_abs)
        np.testing.assert_allclose(td, td64, rtol=GRAD_TOL, atol=GRAD_TOL)
        slots = per.slots.cpu().numpy()
        np.testing.assert_allclose(_np(per.leaves)[slots],
                                   (_stored_td(slots, td) + EPS) ** ALPHA, rtol=LEAF_RTOL, atol=0)
        _check_tree(per)
        assert float(per.max_priority.item()) >= np.float32(td.max())


def test_prioritized_dqn_fit(device, tmp_path):
    """fit() over 200 steps: it runs, the losses are finite, beta annealed on the device, the
    tree stayed consistent."""
    agent = _dqn(device, tmp_path, prioritized=True, per_beta_steps=400, epsilon_start=1.0,
                 epsilon_decay_steps=100)
    agent.fit(max_steps=200)
    torch.cuda.synchronize()
    assert agent.steps >= 200
    assert int(agent.model.optimizer.iterations.item()) == agent.steps // 4
    assert torch.isfinite(agent.td_loss).all() and torch.isfinite(agent.model.theta).all()
    beta = 0.4 + 0.6 * (agent.steps - 4) / 400
    assert agent.per_beta == pytest.approx(beta)
    assert float(agent.per.beta.item()) == np.float32(beta)
    leaves, root = _check_tree(agent.per)
    assert root > 0 and np.isfinite(leaves).all()
    assert np.count_nonzero(leaves) == int(np.minimum(agent.replay.host_count, 16).sum())


def _sac(device, **kwargs):
    from xagents_amd import SAC
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    np.random.seed(0)
    random.seed(0)
    n = 4
    env_kwargs = kwargs.pop('env_kwargs', {})
    envs = create_envs('Pendulum-v1', n, device=device, seed=4, **env_kwargs)
    kw = dict(seed=7, device=device, optimizer_kwargs=dict(learning_rate=1e-3))
    actor = create_model(envs, 'sac', 'actor_model', **kw)
    critic = create_model(envs, 'sac', 'critic_model', **kw)
    bufs = create_buffers('sac', 8 * n, 2 * n, n, initial_size=4 * n)
    agent = SAC(envs, actor, critic, bufs, gradient_steps=1, tau=0.05, seed=3, quiet=True,
                gamma=0.99, **kwargs)
    # a seeded model draws critic 2 equal to critic 1 (every min would tie): move it
    g = torch.Generator().manual_seed(1)
    scale = 1.0 + 0.2 * torch.randn(agent.critic2.n_params, generator=g)
    agent.critic2.theta.mul_(scale.to(device))
    agent.target_critic2.theta.copy_(agent.critic2.theta)
    return agent


def _sac_state(agent):
    ts = [m.theta for m in (agent.actor, agent.critic1, agent.critic2, agent.target_critic1,
                            agent.target_critic2)] + [agent.log_alpha, agent.rng_counter]
    return [t.cpu().numpy().tobytes() for t in ts]


def test_prioritized_sac_with_beta_zero_equals_plain(device):
    per, plain = _sac(device, prioritized=True, per_beta=0.0), _sac(device)
    assert per.batch_size == 8 and per.per is not None and plain.per is None
    for agent in (per, plain):
        _fill(agent)
    assert _sac_state(per) == _sac_state(plain)
    assert per.replay.actions.cpu().numpy().tobytes() == plain.replay.actions.cpu().numpy().tobytes()
    for _ in range(3):  # eager, capturing and replayed passes of the captured phases
        per.update_weights(1)
        torch.cuda.synchronize()
        slots = per.per.slots.cpu().numpy().copy()
        assert (per.per.weights.cpu().numpy() == 1.0).all()
        plain.replay.sample_slots = lambda s=slots: s
        plain.update_weights(1)
        torch.cuda.synchronize()
        assert per.s.cpu().numpy().tobytes() == plain.s.cpu().numpy().tobytes()
    assert _sac_state(per) == _sac_state(plain)
    assert int(per.per.counter.item()) == 3
    assert int(per.critic1.optimizer.iterations.item()) == 3


def test_prioritized_sac_gradient_vs_f64(device):
    """beta = 0.4: both critics' raw gradients are the f64 per-sample gradients combined with
    the device's weights; the priority is the twins' mean |TD error| (rows of one transition
    draw different next actions, so a slot sampled twice has two: its last item's is kept)."""
    import nets_f64 as O
    import sac_ref as S
    agent = _sac(device, prioritized=True, per_beta=0.4)
    _fill(agent)
    per = agent.per
    _spread_priorities(per)
    act, crit = agent.actor, agent.critic
    out = crit.outputs[0]
    for k in range(3):
        th = [_np(m.theta) for m in (agent.actor, agent.critic1, agent.critic2)]
        tt = [_np(agent.target_critic1.theta), _np(agent.target_critic2.theta)]
        la = float(agent.log_alpha.item())
        agent.update_weights(1)
        torch.cuda.synchronize()
        w = _np(per.weights)
        assert w.max() == 1.0 and (w > 0).all() and w.min() < 1.0
        s, a, r, d, s2 = (_np(x) for x in (agent.s, agent.a, agent.r, agent.d, agent.s2))
        B = s.shape[0]
        o2 = S._fw(act, th[0], s2)[1]
        a2, logp2, _ = S.sample(o2[act.outputs[0]], o2[act.outputs[1]], _np(agent.eps_next))
        s2a2 = np.concatenate([s2, a2], 1)
        tv = [S._fw(crit, t, s2a2)[1][out][:, 0] for t in tt]
        sa = np.concatenate([s, a], 1)
        fwd = [S._fw(crit, th[i], sa) for i in (1, 2)]
        v = [o[out][:, 0] for _, o in fwd]
        dv = S.td_grad(v[0], v[1], tv[0], tv[1], logp2, la, r, d, 0.99, 0.0)[:2]
        y = S.soft_target(r, d, 0.99, tv[0], tv[1], la, logp2)
        for i, got in ((0, agent.g_critic), (1, agent.g_critic2)):
            x64, o = fwd[i]
            g = np.zeros(crit.n_params)
            for b in range(B):
                one = np.zeros((B, 1))
                one[b, 0] = dv[i][b]
                g += w[b] * O.backward(crit.layers, th[i + 1], x64, o, {out: one})
            e = _rel(_np(got), g)
            assert e < GRAD_TOL, f'step {k}: critic {i + 1} raw gradient {e:.2e}'
        td64 = 0.5 * (np.abs(v[0] - y) + np.abs(v[1] - y))
        td = _np(per.td_abs)
        np.testing.assert_allclose(td, td64, rtol=GRAD_TOL, atol=GRAD_TOL)
        slots = per.slots.cpu().numpy()
        np.testing.assert_allclose(_np(per.leaves)[slots],
                                   (_stored_td(slots, td) + EPS) ** ALPHA, rtol=LEAF_RTOL, atol=0)
        _check_tree(per)


def test_prioritized_sac_fit(device):
    """fit() over 200 steps on 10-step episodes: every finished episode runs a prioritized
    gradient step; parameters and losses stay finite, beta annealed."""
    agent = _sac(device, prioritized=True, per_beta_steps=400,
                 env_kwargs=dict(max_episode_steps=10))
    agent.fit(max_steps=200)
    torch.cuda.synchronize()
    it = int(agent.critic1.optimizer.iterations.item())
    assert it > 0 and it == agent.games and int(agent.per.counter.item()) == it
    for m in (agent.actor, agent.critic1, agent.critic2):
        assert torch.isfinite(m.theta).all()
    assert torch.isfinite(agent.critic_loss).all() and np.isfinite(agent.alpha)
    assert 0.4 < agent.per_beta <= 1.0
    assert float(agent.per.beta.item()) == np.float32(agent.per_beta)
    leaves, root = _check_tree(agent.per)
    assert root > 0 and np.isfinite(leaves).all()
    assert np.count_nonzero(leaves) == int(agent.replay.host_count.sum())
