"""Host checks of Soft Actor-Critic: the float64 restatement (tests/sac_ref.py) against
central finite differences of its own losses, the overflow-free log-density, the clamp's
derivative, the registry entry, the .cfg models and the C ABI of the new entry points."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import sac_ref as R

ROOT = Path(__file__).resolve().parents[1]
SAC_SYMBOLS = ('xa_sac_sample', 'xa_sac_td_grad', 'xa_sac_actor_seed', 'xa_sac_head_grad')


def _fd(f, x, h=1e-6):
    """Central finite differences of the scalar f over every element of x."""
    g = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (f(xp) - f(xm)) / (2 * h)
    return g


def _critic(a, w):
    """A smooth stand-in critic q(a) [B] with its gradient, per row."""
    return np.sin(a @ w) + 0.3 * (a * a).sum(1), np.cos(a @ w)[:, None] * w + 0.6 * a


@pytest.mark.parametrize('A', [1, 4])
def test_head_gradient_matches_finite_differences(A):
    """dmean / dlog_std of mean(alpha logp - min(q1, q2)(tanh(u))) with the critic seeds on
    the minimum, log_std inside the clamp."""
    rng = np.random.default_rng(A)
    B = 7
    mean, log_std = rng.normal(size=(B, A)), rng.uniform(-3, 1, size=(B, A))
    eps = rng.normal(size=(B, A))
    w1, w2 = rng.normal(size=A), rng.normal(size=A)
    log_alpha = -0.4

    def loss(m, ls):
        a, logp, _ = R.sample(m, ls, eps)
        return R.actor_rows(_critic(a, w1)[0], _critic(a, w2)[0], logp, log_alpha).mean()

    a, _, _ = R.sample(mean, log_std, eps)
    (q1, g1), (q2, g2) = _critic(a, w1), _critic(a, w2)
    dq1, dq2 = R.actor_seed(q1, q2)
    assert np.all((dq1 == 0) != (dq2 == 0)) and np.allclose(dq1 + dq2, -1.0 / B)
    dqa = dq1[:, None] * g1 + dq2[:, None] * g2
    dmean, dlog_std = R.head_grad(dqa, a, eps, log_std, log_alpha)
    np.testing.assert_allclose(dmean, _fd(lambda m: loss(m, log_std), mean), rtol=1e-6,
                               atol=1e-8)
    np.testing.assert_allclose(dlog_std, _fd(lambda ls: loss(mean, ls), log_std), rtol=1e-6,
                               atol=1e-8)


def test_critic_seeds_and_tie():
    """The seeds are the derivative of -mean(min(q1, q2)) away from ties; a tie goes to
    critic 1."""
    rng = np.random.default_rng(3)
    q1, q2 = rng.normal(size=9), rng.normal(size=9)
    dq1, dq2 = R.actor_seed(q1, q2)
    f = lambda a, b: -np.minimum(a, b).mean()  # noqa: E731
    np.testing.assert_allclose(dq1, _fd(lambda x: f(x, q2), q1), atol=1e-9)
    np.testing.assert_allclose(dq2, _fd(lambda x: f(q1, x), q2), atol=1e-9)
    q2[4] = q1[4]
    dq1, dq2 = R.actor_seed(q1, q2)
    assert dq1[4] == -1.0 / 9 and dq2[4] == 0.0


@pytest.mark.parametrize('delta', [0.0, 0.5])
def test_td_gradient_matches_finite_differences(delta):
    rng = np.random.default_rng(5)
    B = 11
    v1, v2, tv1, tv2, logp2, r = (rng.normal(size=B) for _ in range(6))
    done = (rng.random(B) < 0.3).astype(np.float64)
    args = (tv1, tv2, logp2, 0.2, r, done, 0.99, delta)
    total = lambda a, b: R.td_grad(a, b, *args)[2].sum()  # noqa: E731
    d1, d2, _ = R.td_grad(v1, v2, *args)
    np.testing.assert_allclose(d1, _fd(lambda x: total(x, v2), v1), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(d2, _fd(lambda x: total(v1, x), v2), rtol=1e-6, atol=1e-8)
    # the target is entropy-regularised: y = r + (1 - d) gamma (min tv - alpha logp')
    y = R.soft_target(r, done, 0.99, tv1, tv2, 0.2, logp2)
    want = r + (1 - done) * 0.99 * (np.minimum(tv1, tv2) - np.exp(0.2) * logp2)
    np.testing.assert_allclose(y, want, rtol=1e-15)


def test_temperature_gradient_matches_finite_differences():
    rng = np.random.default_rng(6)
    logp = rng.normal(size=13) * 3
    g = _fd(lambda la: R.temperature_loss(la[0], logp, -4.0), np.array([0.3]))[0]
    np.testing.assert_allclose(R.temperature_grad(logp, -4.0), g, rtol=1e-8)


def test_stable_log_density_term():
    """2 (log 2 - u - softplus(-2u)) equals log(1 - tanh(u)^2) for |u| <= 3 and stays finite
    (the naive form is -inf there) for |u| up to 20."""
    u = np.linspace(-3, 3, 601)
    np.testing.assert_allclose(R.log_one_minus_tanh2(u), R.log_one_minus_tanh2_naive(u),
                               rtol=1e-12, atol=1e-13)
    big = np.array([-20.0, -19.5, -12.0, 12.0, 19.5, 20.0])
    got = R.log_one_minus_tanh2(big)
    assert np.all(np.isfinite(got))
    # 1 - tanh^2 u -> 4 exp(-2 |u|)
    np.testing.assert_allclose(got, np.log(4.0) - 2 * np.abs(big), atol=1e-9)
    with np.errstate(divide='ignore'):
        assert not np.all(np.isfinite(R.log_one_minus_tanh2_naive(big)))
    _, logp, _ = R.sample(big[None], np.zeros((1, 6)), np.zeros((1, 6)))
    assert np.isfinite(logp).all()


def test_log_std_gradient_is_zero_outside_the_clamp():
    rng = np.random.default_rng(8)
    log_std = np.array([[-25.0, -20.0, -3.0, 2.0, 2.5]])
    dqa, eps = rng.normal(size=(1, 5)), rng.normal(size=(1, 5))
    a, _, _ = R.sample(np.zeros((1, 5)), log_std, eps)
    dmean, dlog_std = R.head_grad(dqa, a, eps, log_std, 0.1)
    assert dlog_std[0, 0] == 0.0 and dlog_std[0, 4] == 0.0
    assert np.all(dlog_std[0, 1:4] != 0.0) and np.all(dmean != 0.0)
    np.testing.assert_array_equal(R.clamp_grad(log_std), [[0, 1, 1, 1, 0]])
    np.testing.assert_array_equal(R.clamp_log_std(log_std), [[-20, -20, -3, 2, 2]])


def test_registry_entry():
    import xagents_amd
    entry = xagents_amd.agents['sac']
    assert entry['agent'] is xagents_amd.SAC and issubclass(xagents_amd.SAC, xagents_amd.OffPolicy)
    assert entry['actor_model']['ann'] and entry['critic_model']['ann']
    assert Path(entry['actor_model']['ann'][0]).name == 'ann-actor.cfg'
    assert Path(entry['critic_model']['ann'][0]).name == 'ann-critic.cfg'


@pytest.mark.parametrize('env_id,S,A', [('Pendulum-v1', 3, 1), ('BipedalWalker-v3', 24, 4)])
def test_cfgs_parse(env_id, S, A):
    """The actor: two linear n_actions-wide outputs [mean, log_std] on a shared trunk; the
    critic: [state, action] -> 1."""
    import xagents_amd
    from xagents_amd.nets import ModelReader
    entry = xagents_amd.agents['sac']
    actor = ModelReader(entry['actor_model']['ann'][0], [A, A], (S,))._parse()
    outs = [l for l in actor if l.output]
    assert len(outs) == 2 and [l.units for l in outs] == [A, A]
    assert all(l.activation in (None, 'linear') and l.kind == 'dense' for l in outs)
    trunk = [i for i, l in enumerate(actor) if l.common]
    assert len(trunk) == 1 and all(l.input_index == trunk[0] for l in outs)
    critic = ModelReader(entry['critic_model']['ann'][0], [1], (S + A,))._parse()
    assert critic[0].in_features == S + A
    assert [l.units for l in critic if l.output] == [1]


def test_data_parallel_is_refused(monkeypatch):
    """Inside an initialised process group the constructor raises before it touches its
    arguments, unless data_parallel=False asks for an independent agent per process."""
    import torch.distributed as dist
    from xagents_amd import SAC
    monkeypatch.setattr(dist, 'is_available', lambda: True)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    for kw in ({}, dict(data_parallel=None), dict(data_parallel=True)):
        with pytest.raises(NotImplementedError, match='data-parallel'):
            SAC(None, None, None, None, **kw)
    with pytest.raises(AttributeError):  # past the guard: the (absent) actor is inspected
        SAC(None, None, None, None, data_parallel=False)


def test_abi_symbols_resolve_with_declared_types():
    """Every xa_sac_* entry point is declared in the header with as many parameters as the
    ctypes signature, and resolves in the loaded library."""
    from xagents_amd import _lib
    header = (ROOT / 'include' / 'xagents_hip.h').read_text()
    lib = _lib.load()
    for name in SAC_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        res, args = _lib._SIGNATURES[name]
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert m, f'{name} is not declared in xagents_hip.h'
        params = [p.strip() for p in m.group(1).split(',')]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):
            if '*' in p:
                assert t is ctypes.c_void_p, (name, p)
            elif p.startswith('int64_t'):
                assert t is ctypes.c_int64, (name, p)
            elif p.startswith('uint64_t'):
                assert t is ctypes.c_uint64, (name, p)
            elif p.startswith('float'):
                assert t is ctypes.c_float, (name, p)
            else:
                assert p.startswith('int ') and t is ctypes.c_int, (name, p)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
