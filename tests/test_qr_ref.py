"""CPU tests of the float64 restatement of QR-DQN's head (tests/qr_ref.py) -- its gradient
against finite differences, the N = 1 and done reductions, the generator's guarantees at the
shapes the GPU tests use -- and of the host surface the agent adds (registry, create_model's
unit rule, argument checks)."""
import numpy as np
import pytest

import qr_ref as R


def _args(c, double, kappa):
    return (c['next_t'], c['next_o'] if double else None, c['act'], c['rew'], c['done'],
            R.GAMMA, kappa, c['A'], c['N'])


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('kappa', R.KAPPAS)
@pytest.mark.parametrize('B,A,N', [(3, 2, 5), (1, 3, 2), (4, 1, 1)])
def test_gradient_equals_central_differences(B, A, N, kappa, double, weighted):
    """Every entry of dtheta against (f(theta + h e) - f(theta - h e)) / 2h of the batch-mean
    loss, h = 1e-6.

    Each pair's rho is piecewise quadratic / linear in theta_i, so the central difference is
    exact except for rounding and for pairs with a kink (u = 0, where the weight switches
    between tau and 1 - tau, or |u| = kappa) inside the step. At a kink between second
    derivatives a and b the central difference is off by |a - b| h / 4 <= h / (4 kappa) per
    pair before the 1 / (N B) scaling; a done row has all N targets equal, so up to N pairs
    of one theta_i can sit on a kink at once (the generator puts theta[0][a_0][0] there):
    <= h / (4 kappa B). Rounding: two evaluations of a loss of size F, each good to a few
    eps64 F, over 2h: 4 eps64 F / h. h = 1e-6 keeps both near 1e-6 / B and 1e-9."""
    c = R.case(B, A, N, kappa, seed=1)
    args = _args(c, double, kappa)
    w = c['weights'] if weighted else None
    theta = c['theta'].astype(np.float64)
    got = R.td(theta, *args, weights=w)['dtheta']
    h = 1e-6
    F = abs(R.batch_mean_loss(theta, *args, weights=w))
    tol = h / (4 * kappa * B) + 4 * 2.0 ** -52 * max(F, 1.0) / h
    fd = np.zeros_like(theta)
    for b in range(B):
        for e in range(A * N):
            hi, lo = theta.copy(), theta.copy()
            hi[b, e] += h
            lo[b, e] -= h
            fd[b, e] = (R.batch_mean_loss(hi, *args, weights=w) -
                        R.batch_mean_loss(lo, *args, weights=w)) / (2 * h)
    assert np.abs(got).max() > 1e-3 / B
    assert np.abs(got - fd).max() <= tol
    # no gradient off the taken action
    off = np.ones((B, A, N), bool)
    off[np.arange(B), c['act']] = False
    assert (got.reshape(B, A, N)[off] == 0).all() and (fd.reshape(B, A, N)[off] == 0).all()


@pytest.mark.parametrize('kappa', R.KAPPAS)
def test_single_quantile_reduces_to_half_huber(kappa):
    """N = 1: tau_hat = 0.5 whatever the sign of u, so loss = 0.5 Huber(y - theta) / kappa and
    dtheta = -0.5 clip(u, +-kappa) / kappa / B."""
    B, A = 9, 3
    c = R.case(B, A, 1, kappa)
    r = R.td(c['theta'], *_args(c, True, kappa))
    u = r['y'][:, 0] - c['theta'].astype(np.float64)[np.arange(B), c['act']]
    L, Lp = R.huber(u, kappa)
    np.testing.assert_allclose(r['loss'], 0.5 * L / kappa, rtol=1e-15, atol=0)
    np.testing.assert_allclose(r['dtheta'][np.arange(B), c['act']], -0.5 * Lp / kappa / B,
                               rtol=1e-15, atol=0)
    np.testing.assert_allclose(r['td_abs'], np.abs(u), rtol=1e-15, atol=0)


def test_done_rows_target_the_reward():
    c = R.case(65, 6, 2, 1.0)
    _, y = R.targets(c['next_t'], None, c['rew'], c['done'], R.GAMMA, 6, 2)
    d = c['done'] != 0
    assert d.any() and not d.all()
    assert (y[d] == c['rew'][d].astype(np.float64)[:, None]).all()
    assert (y[~d] != c['rew'][~d].astype(np.float64)[:, None]).all()


@pytest.mark.parametrize('kappa', R.KAPPAS)
@pytest.mark.parametrize('B,A,N', R.SHAPES)
def test_generator_margins_hold_at_every_gpu_shape(B, A, N, kappa):
    c = R.case(B, A, N, kappa)  # (asserts them itself)
    R.check_case(c, kappa)
    for key in ('theta', 'next_t', 'next_o'):
        assert c[key].dtype == np.float32 and c[key].shape == (B, A * N)
        assert R.margin(c[key], A, N) >= R.MARGIN
    for online in (None, c['next_o']):
        u = R.td(c['theta'], c['next_t'], online, c['act'], c['rew'], c['done'], R.GAMMA,
                 kappa, A, N)['u']
        assert (np.abs(u) > kappa).any() and (np.abs(u) < kappa).any() and (u == 0).any()
    assert c['done'][0] == 1
    b = R.bounds(c, kappa)
    # (the derived bounds stay far below what they bound: 1 / B, and N S for the loss)
    assert all(v > 0 for v in b.values()) and b['grad'] * B < 1e-4 and b['loss'] < 1e-4 * N * 4


def test_gpu_shapes_cover_every_asked_value():
    assert {s[0] for s in R.SHAPES} == {1, 5, 65}
    assert {s[1] for s in R.SHAPES} == {1, 2, 6}
    assert {s[2] for s in R.SHAPES} == {1, 2, 63, 64, 65, 200, 256}


def test_generator_refuses_the_one_pair_shape():
    with pytest.raises(AssertionError, match='one pair'):
        R.case(1, 2, 1, 1.0)


# ---- host surface --------------------------------------------------------------------------
def _env(obs=(4,), n=2):
    from xagents_amd.envs import Box, Discrete

    class E:
        observation_space = Box(-1, 1, obs)
        action_space = Discrete(n)

    return E()


def test_qrdqn_is_registered_with_default_cfgs():
    import xagents_amd
    from xagents_amd import DQN, QRDQN
    entry = xagents_amd.agents['qrdqn']
    assert entry['agent'] is QRDQN and issubclass(QRDQN, DQN)
    assert 'QRDQN' in xagents_amd.__all__
    for kind in ('cnn', 'ann'):
        cfgs = entry['model'][kind]
        assert len(cfgs) == 1 and cfgs[0].endswith(f'qrdqn/models/{kind}.cfg')
    assert QRDQN._supports_prioritized


def test_create_model_multiplies_the_output_by_n_quantiles():
    from xagents_amd.utils.common import create_model
    m = create_model(_env(n=3), 'qrdqn', 'model', seed=1, device='cpu', n_quantiles=7)
    assert [l.units for l in m.layers] == [64, 64, 21] and list(m.outputs) == [2]
    assert [l.activation for l in m.layers] == ['relu', 'relu', None]
    m = create_model(_env(n=3), 'qrdqn', 'model', seed=1, device='cpu')
    assert m.layers[-1].units == 3 * 32
    m = create_model(_env(obs=(84, 84, 1), n=6), 'qrdqn', 'model', seed=1, device='cpu',
                     n_quantiles=2)
    assert [l.out_shape for l in m.layers] == [(84, 20, 32), (84, 9, 64), (84, 7, 64), (37632,),
                                               (512,), (12,)]


def test_create_model_for_dqn_is_unchanged():
    """The dqn rule ignores n_quantiles: A output units and the parameters of the seed."""
    from xagents_amd.utils.common import create_model
    env = _env(obs=(84, 84, 1), n=6)
    a = create_model(env, 'dqn', 'model', seed=3, device='cpu')
    b = create_model(env, 'dqn', 'model', seed=3, device='cpu', n_quantiles=7)
    for m in (a, b):
        assert m.layers[-1].units == 6 and m.n_params == 288 + 8256 + 12352 + 19_268_096 + 3078
    np.testing.assert_array_equal(a.theta.numpy(), b.theta.numpy())
    m = create_model(_env(), 'ppo', 'model', seed=55, device='cpu', n_quantiles=7)
    assert m.n_params == 4675


@pytest.mark.parametrize('kappa', [0.0, -1.0, float('nan')])
def test_non_positive_huber_kappa_raises(kappa):
    """Checked before anything is built, so no env or device is needed."""
    from xagents_amd import QRDQN
    with pytest.raises(ValueError, match='huber_kappa'):
        QRDQN(None, None, None, huber_kappa=kappa)


def test_huber_delta_is_rejected():
    from xagents_amd import QRDQN
    with pytest.raises(TypeError, match='huber_kappa'):
        QRDQN(None, None, None, huber_delta=1.0)


def test_entry_points_refuse_illegal_shapes_on_the_host():
    """N = 257, N = 0, A = 0 and kappa <= 0 are refused before any device call (so this runs
    without a GPU) with a message."""
    from xagents_amd import _lib
    lib = _lib.load()
    p = 64  # any non-null address: nothing is launched
    td = lambda A, N, kappa: lib.xa_qr_td_grad(p, p, None, p, p, p, 4, A, N, 0.99, kappa, p,
                                               None, None, None, None, None)
    assert td(2, 257, 1.0) != 0 and b'n_quantiles <= 256' in lib.xa_last_error()
    assert td(2, 0, 1.0) != 0 and td(0, 8, 1.0) != 0
    assert td(2, 8, 0.0) != 0 and b'huber_kappa' in lib.xa_last_error()
    assert td(2, 8, -0.5) != 0 and td(2, 8, float('nan')) != 0
    assert lib.xa_qr_act(p, 4, 2, 257, None, 0, p, None, None) != 0
    assert b'n_quantiles <= 256' in lib.xa_last_error()
    assert lib.xa_qr_act(None, 4, 2, 8, None, 0, p, None, None) != 0
