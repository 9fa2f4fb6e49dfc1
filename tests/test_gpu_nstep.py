"""GPU tests of n-step replay (csrc/nstep_terms.hpp): xa_ring_gather_nstep bit for bit against
the f32 restatement (tests/nstep_ref.py) over every valid slot of host-written rings, the
per-sample-discount TD heads xa_dqn_td_grad_n / xa_qr_td_grad_n, the error codes, and the DQN /
QRDQN agents with n_steps = 3 (gathered batch against the restatement, raw gradient against the
f64 network oracle, the captured learner phase, the constructor's refusals).

Tolerances:
* the gather: none, every output byte equals the f32 restatement's;
* the heads with null or all-gamma discounts: none, the bytes of the existing entry points;
* xa_qr_td_grad_n with per-row gamma^m: qr_ref.bounds, unchanged (y = v g + r keeps its
  2 eps (|v| + |r|) for any g <= 1);
* xa_dqn_td_grad_n with per-row gamma^m: tests/test_gpu_configs.py's dq error model, per row
  sum |dq - dq64| <= 1e-5 sum |dq64| + 8 * 2^-23 * (|y| + |Q(s, a)|) * 2 / A (the f32 diff
  carries a few ulps of |y| + |Q|, and |y| does not grow with a discount <= 1); Huber's clip is
  1-Lipschitz in the diff, so the same limit holds for it;
* raw gradients through the layer executor: the project's 1e-4 relative.
"""
import ctypes
import functools
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import nstep_ref as NS
import qr_ref as R

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / 'oracle'))
pytestmark = pytest.mark.gpu

GAMMA = np.float32(0.99)
GRAD_TOL = 1e-4
SENTINEL = 0x5A


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


# ---- 1. the gather against the f32 restatement -------------------------------------------------
def _newest(count, cap):
    return (np.asarray(count) - 1) % cap


def _done_rows(pattern, count, cap):
    """dones [n, cap] of a named pattern (ring slots, not walk steps: every valid slot is
    sampled, so each pattern meets walks that start before, at and behind its dones)."""
    n = len(count)
    d = np.zeros((n, cap), np.float32)
    if pattern == 'sampled':  # every walk ends at its own first slot
        d[:] = 1.0
    elif pattern == 'mid':
        d[:, cap // 2] = 1.0
    elif pattern == 'newest':
        d[np.arange(n), _newest(count, cap)] = 1.0
    elif pattern == 'two':
        d[:, [2 % cap, 4 % cap]] = 1.0
    else:
        assert pattern == 'none'
    return d


PATTERNS = ('none', 'sampled', 'mid', 'newest', 'two')


def _rings(rng, n, cap, obs_bytes, act_bytes, count, pattern):
    return dict(states=rng.integers(0, 256, (n, cap, obs_bytes), dtype=np.uint8),
                new_states=rng.integers(0, 256, (n, cap, obs_bytes), dtype=np.uint8),
                actions=rng.integers(0, 256, (n, cap, act_bytes), dtype=np.uint8),
                rewards=rng.normal(size=(n, cap)).astype(np.float32),
                dones=_done_rows(pattern, count, cap))


def _valid_slots(count, cap):
    return np.concatenate([e * cap + np.arange(min(int(c), cap)) for e, c in enumerate(count)])


class _Gather:
    """Device copies of host rings and sentinel-filled destinations with one guard row."""

    def __init__(self, device, rings, count, slots, pinned):
        from xagents_amd import _lib
        self.lib = _lib
        self.t = {k: _dev(device, v) for k, v in rings.items()}
        self.count = _dev(device, np.asarray(count, np.int64))
        self.n_items = n = len(slots)
        self.cap = rings['rewards'].shape[1]
        self.obs_bytes, self.act_bytes = rings['states'].shape[2], rings['actions'].shape[2]
        if pinned:
            self.slots_host, self.slots_ptr = _lib.mapped_pinned(n, torch.int64)
            self.slots_host.numpy()[:] = slots
        else:
            self.slots_dev = _dev(device, np.asarray(slots, np.int64))
            self.slots_ptr = self.slots_dev.data_ptr()
        self.device = device

    def _out(self):
        n, dev = self.n_items + 1, self.device
        u8 = lambda w: torch.full((n, w), SENTINEL, dtype=torch.uint8, device=dev)  # noqa: E731
        f32 = lambda: torch.full((n,), 7.0, dtype=torch.float32, device=dev)  # noqa: E731
        return dict(states=u8(self.obs_bytes), new_states=u8(self.obs_bytes),
                    actions=u8(self.act_bytes), rewards=f32(), dones=f32(), discounts=f32())

    def _check_guard(self, o):
        n = self.n_items
        for k in ('states', 'new_states', 'actions'):
            assert (o[k][n] == SENTINEL).all(), k
        for k in ('rewards', 'dones', 'discounts'):
            assert o[k][n] == 7.0, k
        return {k: v[:n] for k, v in o.items()}

    def nstep_args(self, o, n_steps, kind=None, capacity=None):
        a, t = self.lib.XaNstepGatherArgs(), self.t
        a.ring_states, a.ring_new_states = t['states'].data_ptr(), t['new_states'].data_ptr()
        a.ring_actions = t['actions'].data_ptr()
        a.ring_rewards, a.ring_dones = t['rewards'].data_ptr(), t['dones'].data_ptr()
        a.ring_count = self.count.data_ptr()
        a.obs_bytes, a.act_bytes = self.obs_bytes, self.act_bytes
        a.capacity = self.cap if capacity is None else capacity
        a.ring_kind = self.lib.XA_RING_DEQUE if kind is None else kind
        a.n_steps, a.n_items, a.gamma = n_steps, self.n_items, float(GAMMA)
        a.slots = self.slots_ptr
        a.states, a.actions, a.new_states = \
            o['states'].data_ptr(), o['actions'].data_ptr(), o['new_states'].data_ptr()
        a.rewards, a.dones = o['rewards'].data_ptr(), o['dones'].data_ptr()
        a.discounts = o['discounts'].data_ptr()
        return a

    def nstep(self, n_steps):
        o = self._out()
        _call('xa_ring_gather_nstep', ctypes.byref(self.nstep_args(o, n_steps)))
        return self._check_guard({k: v.cpu().numpy() for k, v in o.items()})

    def fields(self):
        o = self._out()
        a, t = self.lib.XaGatherArgs(), self.t
        pairs = (('states', self.obs_bytes), ('new_states', self.obs_bytes),
                 ('actions', self.act_bytes), ('rewards', 4), ('dones', 4))
        for f, (k, nb) in enumerate(pairs):
            a.field[f].ring, a.field[f].dst, a.field[f].item_bytes = \
                t[k].data_ptr(), o[k].data_ptr(), nb
        a.n_fields, a.n_items, a.slots = len(pairs), self.n_items, self.slots_ptr
        _call('xa_ring_gather_fields', ctypes.byref(a))
        return self._check_guard({k: v.cpu().numpy() for k, v in o.items()})


def _assert_bits(got, want, what):
    for k in ('states', 'actions', 'rewards', 'dones', 'new_states', 'discounts'):
        assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (what, k)


def _two_dones_in_window(rings, count, slots, n_steps):
    cap = rings['rewards'].shape[1]
    for s in slots.tolist():
        e, i = divmod(s, cap)
        m_max, _ = NS.walk(int(count[e]), cap, i, n_steps, rings['dones'][e])
        if sum(rings['dones'][e, (i + k) % cap] != 0 for k in range(m_max)) >= 2:
            return True
    return False


@pytest.mark.parametrize('pinned', [False, True], ids=['device_slots', 'pinned_slots'])
@pytest.mark.parametrize('act_bytes', [4, 16])
@pytest.mark.parametrize('obs_bytes', [4, 20, 28224])
def test_gather_nstep_bit_exact_over_every_valid_slot(device, obs_bytes, act_bytes, pinned):
    """3 envs, capacity 7, counters out of {1, 5, 7, 12} (12: wrapped), every done pattern,
    n_steps in {1, 2, 3, 5, 7}: every output equals the f32 restatement's bytes."""
    n, cap = 3, 7
    rng = np.random.default_rng(obs_bytes + act_bytes + pinned)
    seen_L, seen_two = set(), False
    for count in ((1, 5, 12), (7, 12, 5)):
        slots = _valid_slots(count, cap)
        for pattern in PATTERNS:
            rings = _rings(rng, n, cap, obs_bytes, act_bytes, count, pattern)
            g = _Gather(device, rings, count, slots, pinned)
            for n_steps in (1, 2, 3, 5, 7):
                want = NS.gather(rings, np.asarray(count), slots, n_steps, GAMMA, np.float32)
                got = g.nstep(n_steps)
                _assert_bits(got, want, (count, pattern, n_steps))
                seen_L |= set(want['L'].tolist())
                if pattern == 'two':
                    seen_two |= _two_dones_in_window(rings, count, slots, n_steps)
                if pattern == 'sampled':
                    assert (want['L'] == 0).all() and (got['dones'] == 1.0).all()
                if pattern == 'none':
                    assert (got['dones'] == 0.0).all()
    assert seen_L == set(range(7)) and seen_two


def test_gather_nstep_64_steps_on_a_wrapped_ring(device):
    """n_steps = 64 at capacity 64: counters 100 (wrapped), 64 (just full) and 30."""
    n, cap, count = 3, 64, (100, 64, 30)
    rng = np.random.default_rng(64)
    slots = _valid_slots(count, cap)
    for pattern in ('none', 'two', 'newest'):
        rings = _rings(rng, n, cap, 20, 4, count, pattern)
        if pattern == 'two':
            rings['dones'][:] = 0.0
            rings['dones'][:, [10, 50]] = 1.0
        want = NS.gather(rings, np.asarray(count), slots, 64, GAMMA, np.float32)
        got = _Gather(device, rings, count, slots, pinned=True).nstep(64)
        _assert_bits(got, want, pattern)
        if pattern == 'none':  # the oldest entry of each env walks to the newest
            assert [int(want['L'][slots // cap == e].max()) for e in range(n)] == [63, 63, 29]


@pytest.mark.parametrize('obs_bytes,act_bytes', [(4, 4), (20, 16), (28224, 4)])
def test_gather_nstep_one_step_is_the_plain_gather(device, obs_bytes, act_bytes):
    n, cap, count = 3, 7, (5, 12, 7)
    rng = np.random.default_rng(obs_bytes)
    slots = rng.permutation(_valid_slots(count, cap))
    rings = _rings(rng, n, cap, obs_bytes, act_bytes, count, 'two')
    g = _Gather(device, rings, count, slots, pinned=False)
    plain, one = g.fields(), g.nstep(1)
    for k in ('states', 'actions', 'rewards', 'dones', 'new_states'):
        assert one[k].tobytes() == plain[k].tobytes(), k
    assert (plain['discounts'] == 7.0).all()  # (not a field of the plain gather)
    assert one['discounts'].tobytes() == np.full(len(slots), GAMMA, np.float32).tobytes()


def test_gather_nstep_error_codes_launch_nothing(device):
    from xagents_amd import _lib
    n, cap, count = 3, 7, (5, 12, 7)
    rng = np.random.default_rng(3)
    slots = _valid_slots(count, cap)
    g = _Gather(device, _rings(rng, n, cap, 20, 4, count, 'none'), count, slots, pinned=False)
    cases = ((dict(n_steps=0), 'n_steps 0'), (dict(n_steps=65), 'n_steps 65'),
             (dict(n_steps=8), 'n_steps 8'),  # > capacity 7
             (dict(n_steps=2, kind=_lib.XA_RING_RB2), 'ring kind'))
    for kw, msg in cases:
        o = g._out()
        with pytest.raises(_lib.HipLibraryError, match=msg):
            _call('xa_ring_gather_nstep', ctypes.byref(g.nstep_args(o, **kw)))
        torch.cuda.synchronize()
        for k, v in o.items():
            v = v.cpu().numpy()
            assert (v == (7.0 if v.dtype == np.float32 else SENTINEL)).all(), (kw, k)


# ---- 2. the TD heads with per-sample discounts ------------------------------------------------
HEAD_B, HEAD_A, HEAD_N = (1, 5, 65), (2, 6), (1, 64, 65)


def _dqn_head(device, c, name, double, huber, weights=False, discounts=None):
    B, A = c['B'], c['A']
    t = {k: _dev(device, c[k]) for k in ('q', 'next_t', 'next_o', 'act', 'rew', 'done',
                                         'weights')}
    dq = torch.full((B + 1, A), 7.0, device=device)
    loss = torch.full((B + 1,), 7.0, device=device)
    td_abs = torch.full((B + 1,), 7.0, device=device)
    step = torch.full((2,), 41, dtype=torch.int32, device=device)
    args = [t['q'].data_ptr(), t['next_t'].data_ptr(), t['next_o'].data_ptr() if double else None,
            t['act'].data_ptr(), t['rew'].data_ptr(), t['done'].data_ptr(), B, A, float(GAMMA),
            float(huber), dq.data_ptr(), loss.data_ptr(), step.data_ptr(),
            t['weights'].data_ptr() if weights else None, td_abs.data_ptr()]
    if name == 'xa_dqn_td_grad_n':
        disc = None if discounts is None else _dev(device, discounts)
        args.append(None if disc is None else disc.data_ptr())
    _call(name, *args)
    assert step.cpu().numpy().tolist() == [42, 41]
    out = dict(dq=dq.cpu().numpy(), loss=loss.cpu().numpy(), td_abs=td_abs.cpu().numpy())
    assert (out['dq'][B] == 7.0).all() and out['loss'][B] == 7.0 and out['td_abs'][B] == 7.0
    return {k: v[:B] for k, v in out.items()}


@pytest.mark.parametrize('huber', [0.0, 0.5])
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('A', HEAD_A)
@pytest.mark.parametrize('B', HEAD_B)
def test_dqn_td_grad_n(device, B, A, double, huber):
    c = NS.dqn_case(B, A)
    base = _dqn_head(device, c, 'xa_dqn_td_grad_w', double, huber, weights=True)
    null = _dqn_head(device, c, 'xa_dqn_td_grad_n', double, huber, weights=True)
    same = _dqn_head(device, c, 'xa_dqn_td_grad_n', double, huber, weights=True,
                     discounts=np.full(B, GAMMA, np.float32))
    for k in base:
        assert null[k].tobytes() == base[k].tobytes() == same[k].tobytes(), k
    # per-row gamma^m against float64, test_gpu_configs.py's dq error model
    disc = NS.step_discounts(B, GAMMA)
    got = _dqn_head(device, c, 'xa_dqn_td_grad_n', double, huber, discounts=disc)
    want = NS.dqn_td(c['q'], c['next_t'], c['next_o'] if double else None, c['act'], c['rew'],
                     c['done'], disc, huber)
    if B > 1:  # the discounts matter: another target than with gamma for some row
        one = NS.dqn_td(c['q'], c['next_t'], c['next_o'] if double else None, c['act'],
                        c['rew'], c['done'], np.full(B, GAMMA, np.float32), huber)
        assert (want['y'] != one['y']).any()
    qa = c['q'].astype(np.float64)[np.arange(B), c['act']]
    scale = (np.abs(want['y']) + np.abs(qa)) * 2 / A
    err = np.abs(got['dq'] - want['dq']).sum(1)
    lim = 1e-5 * np.abs(want['dq']).sum(1) + 8 * 2.0 ** -23 * scale
    print(f'dq err / limit, worst row: {(err / lim).max():.3e} (err {err.max():.3e})')
    assert (err <= lim).all()
    off = np.ones((B, A), bool)
    off[np.arange(B), c['act']] = False
    assert (got['dq'][off] == 0).all()
    e_t = np.abs(got['td_abs'] - want['td_abs'])
    assert (e_t <= 8 * 2.0 ** -23 * (np.abs(want['y']) + np.abs(qa))).all()


@functools.lru_cache(maxsize=None)
def _qr_case(B, A, N, kappa):
    c = NS.qr_case(B, A, N, kappa)
    return c, R.bounds(c, kappa)


def _qr_head(device, c, name, double, kappa, weights=False, discounts=None):
    B, A, N = c['B'], c['A'], c['N']
    t = {k: _dev(device, c[k]) for k in ('theta', 'next_t', 'next_o', 'act', 'rew', 'done',
                                         'weights')}
    d = torch.full((B + 1, A * N), 7.0, device=device)
    loss = torch.full((B + 1,), 7.0, device=device)
    td_abs = torch.full((B + 1,), 7.0, device=device)
    step = torch.full((2,), 41, dtype=torch.int32, device=device)
    args = [t['theta'].data_ptr(), t['next_t'].data_ptr(),
            t['next_o'].data_ptr() if double else None, t['act'].data_ptr(),
            t['rew'].data_ptr(), t['done'].data_ptr(), B, A, N, float(GAMMA), float(kappa),
            d.data_ptr(), loss.data_ptr(), step.data_ptr(),
            t['weights'].data_ptr() if weights else None, td_abs.data_ptr()]
    if name == 'xa_qr_td_grad_n':
        disc = None if discounts is None else _dev(device, discounts)
        args.append(None if disc is None else disc.data_ptr())
    _call(name, *args)
    assert step.cpu().numpy().tolist() == [42, 41]
    out = dict(dtheta=d.cpu().numpy(), loss=loss.cpu().numpy(), td_abs=td_abs.cpu().numpy())
    assert (out['dtheta'][B] == 7.0).all() and out['loss'][B] == 7.0 and out['td_abs'][B] == 7.0
    return {k: v[:B] for k, v in out.items()}


@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('N', HEAD_N)
@pytest.mark.parametrize('A', HEAD_A)
@pytest.mark.parametrize('B', HEAD_B)
def test_qr_td_grad_n(device, B, A, N, double):
    kappa = 1.0
    c, bound = _qr_case(B, A, N, kappa)
    base = _qr_head(device, c, 'xa_qr_td_grad', double, kappa, weights=True)
    null = _qr_head(device, c, 'xa_qr_td_grad_n', double, kappa, weights=True)
    same = _qr_head(device, c, 'xa_qr_td_grad_n', double, kappa, weights=True,
                    discounts=np.full(B, GAMMA, np.float32))
    for k in base:
        assert null[k].tobytes() == base[k].tobytes() == same[k].tobytes(), k
    disc = NS.step_discounts(B, GAMMA)
    got = _qr_head(device, c, 'xa_qr_td_grad_n', double, kappa, discounts=disc)
    want = NS.qr_td(c['theta'], c['next_t'], c['next_o'] if double else None, c['act'],
                    c['rew'], c['done'], disc, kappa, A, N)
    e_g = np.abs(got['dtheta'] - want['dtheta']).max()
    e_l = np.abs(got['loss'] - want['loss']).max()
    e_t = np.abs(got['td_abs'] - want['td_abs']).max()
    print(f'grad err {e_g:.3e} bound {bound["grad"]:.3e}; loss err {e_l:.3e} bound '
          f'{bound["loss"]:.3e}; td_abs err {e_t:.3e} bound {bound["td_abs"]:.3e}')
    assert e_g <= bound['grad'] and e_l <= bound['loss'] and e_t <= bound['td_abs']


# ---- 3. agents -------------------------------------------------------------------------------
MLP_CFG = ('[dense-0]\nunits=32\nactivation=relu\n\n[dense-1]\nunits=16\nactivation=relu\n\n'
           '[dense-2]\noutput=1\n')
NQ = 8


def _agent(device, tmp_path, kind='dqn', cls=None, n=4, buffers=None, **kwargs):
    import xagents_amd
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    np.random.seed(1)
    random.seed(1)
    envs = create_envs('CartPole-v1', n, mode='transitions', device=device, seed=3, t_rec=64)
    cfg = tmp_path / 'ann.cfg'
    cfg.write_text(MLP_CFG)
    extra = dict(n_quantiles=NQ) if kind == 'qrdqn' else {}
    model = create_model(envs, kind, 'model', seed=9, device=device, model_cfg=str(cfg),
                         optimizer_kwargs=dict(learning_rate=1e-3), **extra)
    bufs = buffers or create_buffers(kind, 16 * n, 2 * n, n, initial_size=8 * n)
    kw = dict(seed=2, quiet=True, epsilon_start=0.0, epsilon_end=0.0, gamma=0.99, n_steps=3)
    kw.update(extra)
    kw.update(kwargs)
    cls = cls or (xagents_amd.QRDQN if kind == 'qrdqn' else xagents_amd.DQN)
    return cls(envs, model, bufs, **kw)


def _fill(agent):
    np.random.seed(7)
    random.seed(7)
    agent.fill_buffers()


def _step(agent):
    agent.at_step_start()
    agent.train_step()
    agent.at_step_end()


def _host_rings(agent):
    rp = agent.replay
    return dict(states=rp.states.cpu().numpy(), new_states=rp.new_states.cpu().numpy(),
                actions=rp.actions.cpu().numpy(), rewards=rp.rewards.cpu().numpy(),
                dones=rp.dones.cpu().numpy()), rp.count.cpu().numpy()


def _used_slots(agent):
    if agent.per is not None:
        return agent.per.slots.cpu().numpy().copy()
    return agent._gather_stage().host(0).numpy().copy()


def _f64_grad(agent, th0, tt0, ref64, weights):
    """Raw gradient of the gathered batch in float64: the network oracle's forward / backward
    around the restatement's head gradient (its f64 rewards and discounts)."""
    import nets_f64 as O
    model = agent.model
    B = agent.batch_size
    s, s2 = agent.xb[:B].cpu().numpy(), agent.xb[B:].cpu().numpy()
    L, shape, out = model.layers, model.input_shape, model.outputs[0]
    x64, outs = O.forward(L, th0, s, shape)
    next_t = O.forward(L, tt0, s2, shape)[1][out]
    next_o = O.forward(L, th0, s2, shape)[1][out] if agent.double else None
    act, done = agent.b_act.cpu().numpy(), agent.b_done.cpu().numpy()
    if hasattr(agent, 'n_quantiles'):
        r = NS.qr_td(outs[out], next_t, next_o, act, ref64['rewards'], done,
                     ref64['discounts'], agent.huber_kappa, agent.n_actions, agent.n_quantiles,
                     weights)
        seed = r['dtheta']
    else:
        r = NS.dqn_td(outs[out], next_t, next_o, act, ref64['rewards'], done,
                      ref64['discounts'], agent.huber_delta or 0.0, weights)
        seed = r['dq']
    return O.backward(L, th0, x64, outs, {out: seed}), r


@pytest.mark.parametrize('kind,kwargs', [('dqn', {}), ('dqn', dict(double=True, prioritized=True)),
                                         ('qrdqn', {})],
                         ids=['dqn', 'double_dqn_per', 'qrdqn'])
def test_agent_trains_on_the_n_step_batch(device, tmp_path, kind, kwargs):
    """Three train steps with n_steps = 3: the gathered batch is the restatement applied to
    the rings at the slots the step used, and the raw gradient follows from it."""
    agent = _agent(device, tmp_path, kind, **kwargs)
    assert agent.n_steps == 3 and agent.b_disc.shape == (8,) and agent.replay.cap == 16
    _fill(agent)
    agent.target_model.theta.mul_(0.97)
    agent.write_raw_grad = True
    B = agent.batch_size
    seen_m = set()
    for _ in range(3):
        th0, tt0 = _np(agent.model.theta), _np(agent.target_model.theta)
        agent.at_step_start()
        agent.train_step()
        torch.cuda.synchronize()
        rings, count = _host_rings(agent)
        slots = _used_slots(agent)
        want = NS.gather(rings, count, slots, 3, GAMMA, np.float32)
        got = dict(states=agent.xb[:B], new_states=agent.xb[B:], actions=agent.b_act,
                   rewards=agent.b_rew, dones=agent.b_done, discounts=agent.b_disc)
        for k, v in got.items():
            assert v.cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
        seen_m |= set((want['L'] + 1).tolist())
        ref64 = NS.gather(rings, count, slots, 3, GAMMA, np.float64)
        w = None if agent.per is None else agent.per.weights.cpu().numpy()
        g, r = _f64_grad(agent, th0, tt0, ref64, w)
        e = _rel(_np(agent.grad), g)
        print(f'raw gradient rel err {e:.3e}')
        assert np.abs(g).max() > 0 and e < GRAD_TOL
        np.testing.assert_allclose(_np(agent.td_loss), r['loss'], rtol=GRAD_TOL, atol=GRAD_TOL)
        agent.at_step_end()
    assert 3 in seen_m  # (some sampled slot had three steps ahead of it)
    assert int(agent.model.optimizer.iterations.item()) == 3


def test_n_steps_one_allocates_nothing_and_keeps_the_fused_head(device, tmp_path):
    agent = _agent(device, tmp_path, n_steps=1)
    assert not hasattr(agent, 'b_disc') and agent._nstep() is None and agent._head_fused()
    assert agent._td_entry('a', 'b') == ('a', ())
    three = _agent(device, tmp_path)
    assert three._td_entry('a', 'b') == ('b', (three.b_disc.data_ptr(),))


def test_captured_learner_matches_eager_with_n_steps(device, tmp_path, monkeypatch):
    out = []
    for use_graph in (False, True):
        monkeypatch.setenv('XA_DQN_LEARN_GRAPH', '1' if use_graph else '0')
        agent = _agent(device, tmp_path, double=True, epsilon_start=1.0, epsilon_decay_steps=8,
                       target_sync_steps=8)
        agent.use_graph = use_graph
        _fill(agent)
        np.random.seed(4)
        random.seed(4)
        for _ in range(3):
            _step(agent)
        torch.cuda.synchronize()
        assert (agent._lgraph is not None) == use_graph
        opt = agent.model.optimizer
        out.append([x.cpu().numpy().tobytes() for x in
                    (agent.model.theta, agent.target_model.theta, opt.m, opt.v, opt.iterations,
                     agent.b_rew, agent.b_disc, agent.dq)])
    assert out[0] == out[1]


def test_constructor_refuses_what_the_walk_cannot_serve(device, tmp_path):
    from xagents_amd.utils.buffers import ReplayBuffer2
    rb2 = [ReplayBuffer2(16, 5, initial_size=8, batch_size=2) for _ in range(4)]
    with pytest.raises(ValueError, match='ReplayBuffer1'):
        _agent(device, tmp_path, buffers=rb2, n_steps=2)
    with pytest.raises(ValueError, match='n_steps'):
        _agent(device, tmp_path, n_steps=65)
    with pytest.raises(ValueError, match='n_steps'):
        _agent(device, tmp_path, n_steps=17)  # buffer size 16
    assert _agent(device, tmp_path, n_steps=16).b_disc.shape == (8,)


def test_overridden_hook_with_n_steps_is_refused(device, tmp_path):
    import xagents_amd

    class Hooked(xagents_amd.DQN):
        def get_targets(self, *batch):
            return super().get_targets(*batch)

    agent = _agent(device, tmp_path, cls=Hooked, n_steps=2)
    _fill(agent)
    with pytest.raises(NotImplementedError, match='discounts'):
        agent.train_step()
    assert agent.steps == 0
    one = _agent(device, tmp_path, cls=Hooked, n_steps=1)  # one-step: the composed path as ever
    _fill(one)
    one.train_step()
    torch.cuda.synchronize()
    assert one.steps == one.n_envs
