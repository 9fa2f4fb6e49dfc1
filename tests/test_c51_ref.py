"""CPU tests of the float64 restatement of categorical DQN's head (tests/c51_ref.py) -- the
gather projection against the floor / ceil scatter, its mass and mean, the gradient against
finite differences, the generator's guarantees at the shapes the GPU tests use -- and of the
host surface the agent adds (registry, create_model's unit rule, argument checks)."""
import functools

import numpy as np
import pytest

import c51_ref as R

CASES = [(*s, *v) for s in R.SHAPES for v in R.SUPPORTS]


@functools.lru_cache(maxsize=None)
def _projected(B, A, K, v_min, v_max):
    c = R.case(B, A, K, v_min, v_max)  # (asserts its guarantees itself)
    out = {(d, n): R.target_dist(c['next_t'], c['next_o'] if d else None, c['rew'], c['done'],
                                 R.GAMMA, A, K, v_min, v_max, c['disc'] if n else None)
           for d in (False, True) for n in (False, True)}
    return c, out


@pytest.mark.parametrize('B,A,K,v_min,v_max', CASES)
def test_gather_projection_equals_the_scatter(B, A, K, v_min, v_max):
    """m_i = sum_j p'_j max(0, 1 - |b_j - i|) against Algorithm 1's scatter onto floor(b_j)
    and ceil(b_j), the mass placed whole when they coincide. In exact arithmetic the two are
    equal; in f64 each weight carries a few roundings of values <= K: 1e-12."""
    c, out = _projected(B, A, K, v_min, v_max)
    for r in out.values():
        assert np.abs(r['m'] - R.project_scatter(r['p_next'], r['b'])).max() <= 1e-12
    # the scatter as it is usually written (no l == u branch) loses row 0's whole mass
    r = out[(False, False)]
    lo, up = np.floor(r['b'][0]), np.ceil(r['b'][0])
    assert (lo == up).all() and ((up - r['b'][0]) + (r['b'][0] - lo) == 0).all()
    assert abs(r['m'][0].sum() - 1.0) <= 1e-12


@pytest.mark.parametrize('B,A,K,v_min,v_max', CASES)
def test_projection_keeps_the_mass_and_the_clipped_mean(B, A, K, v_min, v_max):
    c, out = _projected(B, A, K, v_min, v_max)
    z, _ = R.support(K, v_min, v_max)
    scale = max(abs(v_min), abs(v_max))
    for r in out.values():
        assert (r['m'] >= 0).all()
        assert np.abs(r['m'].sum(1) - 1.0).max() <= 1e-12
        mean = (r['p_next'] * np.clip(r['tz'], v_min, v_max)).sum(1)
        assert np.abs((r['m'] * z).sum(1) - mean).max() <= 1e-12 * scale
    if B >= 3:  # rows 1 and 2 clip: mass on the end atoms beyond what the next state put there
        r = out[(False, False)]
        assert r['m'][1, K - 1] > r['p_next'][1, K - 1] and r['m'][2, 0] > r['p_next'][2, 0]
    if (v_min, v_max) == (-1.0, 1.0) and B >= 3:  # |r| = 3: the whole row on one atom
        assert abs(out[(False, False)]['m'][1, K - 1] - 1.0) <= 1e-12
        assert np.abs(c['rew']).max() == 3.0


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('v_min,v_max', R.SUPPORTS)
@pytest.mark.parametrize('B,A,K', [(3, 2, 5), (1, 3, 2), (4, 1, 7)])
def test_gradient_equals_central_differences(B, A, K, v_min, v_max, double, weighted):
    """dtheta B against (f(theta + h e) - f(theta - h e)) / 2h of the sample's loss in every
    logit, h = 1e-5.

    loss[b] = -sum_i m_i log p_i is smooth in the taken action's logits and m does not depend
    on them. Its third derivative along one logit is sum(m) p (1 - p) (1 - 2 p), at most 0.1,
    so the central difference is off by <= 0.1 h^2 / 6; two evaluations of a loss of size F,
    each good to a few eps64 F, over 2h add 4 eps64 F / h; dtheta itself stands for the
    gradient with sum(m) = 1, off by `mass` 2^-29 (c51_ref.bounds)."""
    c = R.case(B, A, K, v_min, v_max, seed=1)
    w = c['weights'] if weighted else None
    args = (c['next_t'], c['next_o'] if double else None, c['act'], c['rew'], c['done'],
            R.GAMMA, A, K, v_min, v_max, w, c['disc'])
    theta = c['theta'].astype(np.float64)
    r = R.td(theta, *args)
    got = r['dtheta'] * B
    h = 1e-5
    tol = 0.1 * h * h / 6 + 4 * 2.0 ** -52 * max(r['loss'].max(), 1.0) / h + \
        R.bounds(c)['mass'] * 2.0 ** -29
    fd = np.zeros_like(theta)
    for b in range(B):
        for e in range(A * K):
            hi, lo = theta.copy(), theta.copy()
            hi[b, e] += h
            lo[b, e] -= h
            fd[b, e] = (R.td(hi, *args)['loss'][b] - R.td(lo, *args)['loss'][b]) / (2 * h)
    assert np.abs(got).max() > 1e-3
    assert np.abs(got - fd).max() <= tol
    # no gradient off the taken action
    off = np.ones((B, A, K), bool)
    off[np.arange(B), c['act']] = False
    assert (got.reshape(B, A, K)[off] == 0).all() and (fd.reshape(B, A, K)[off] == 0).all()


@pytest.mark.parametrize('B,A,K,v_min,v_max', CASES)
def test_generator_guarantees_hold_at_every_gpu_shape(B, A, K, v_min, v_max):
    c, out = _projected(B, A, K, v_min, v_max)
    R.check_case(c)
    for key in ('theta', 'next_t', 'next_o'):
        assert c[key].dtype == np.float32 and c[key].shape == (B, A * K)
        assert R.margin(c[key], A, K, v_min, v_max) >= R.MARGIN
    assert c['done'][0] == 1 and (B == 1 or c['done'][-1] == 0)
    b0 = out[(False, False)]['b'][0]
    assert (b0 == np.round(b0)).all()  # row 0's reward sits on an atom
    if B >= 3:
        tz = out[(False, False)]['tz']
        assert (tz > v_max).any() and (tz < v_min).any()
    g = np.float64(np.float32(R.GAMMA))
    np.testing.assert_allclose(c['disc'], g ** (1 + np.arange(B) % 3), rtol=3 * R.EPS32)
    if B > 1:  # the discounts matter: another target distribution than with gamma
        assert np.abs(out[(False, True)]['m'] - out[(False, False)]['m']).max() > 1e-4
    if A > 1 and B > 1:  # and so does double Q
        assert (out[(True, False)]['a_star'] != out[(False, False)]['a_star']).any()
    bd = R.bounds(c)
    # (the derived bounds stay far below what they bound: probabilities <= 1, |Q| <= V,
    # loss ~ ln K)
    assert all(v > 0 for v in bd.values())
    assert bd['m'] < 1e-3 and bd['grad'] * B < 1e-3 and bd['loss'] < 1e-2
    assert bd['q'] < 1e-3 * max(abs(v_min), abs(v_max)) and bd['td_abs'] < 0.05 * (v_max - v_min)


def test_gpu_shapes_cover_every_asked_value():
    assert {s[0] for s in R.SHAPES} == {1, 5, 65}
    assert {s[1] for s in R.SHAPES} == {1, 2, 6}
    assert {s[2] for s in R.SHAPES} == {2, 51, 63, 64, 65, 200, 256}
    assert R.SUPPORTS == ((-10.0, 10.0), (0.0, 200.0), (-1.0, 1.0))


# ---- host surface --------------------------------------------------------------------------
def _env(obs=(4,), n=2):
    from xagents_amd.envs import Box, Discrete

    class E:
        observation_space = Box(-1, 1, obs)
        action_space = Discrete(n)

    return E()


def test_c51_is_registered_with_default_cfgs():
    import xagents_amd
    from xagents_amd import C51, DQN
    entry = xagents_amd.agents['c51']
    assert entry['agent'] is C51 and issubclass(C51, DQN)
    assert 'C51' in xagents_amd.__all__
    for kind in ('cnn', 'ann'):
        cfgs = entry['model'][kind]
        assert len(cfgs) == 1 and cfgs[0].endswith(f'c51/models/{kind}.cfg')
    assert C51._supports_prioritized


def test_create_model_multiplies_the_output_by_n_atoms():
    from xagents_amd.utils.common import create_model
    m = create_model(_env(n=3), 'c51', 'model', seed=1, device='cpu', n_atoms=7)
    assert [l.units for l in m.layers] == [64, 64, 21] and list(m.outputs) == [2]
    assert [l.activation for l in m.layers] == ['relu', 'relu', None]
    m = create_model(_env(n=3), 'c51', 'model', seed=1, device='cpu')
    assert m.layers[-1].units == 3 * 51
    m = create_model(_env(obs=(84, 84, 1), n=6), 'c51', 'model', seed=1, device='cpu',
                     n_atoms=2)
    assert [l.out_shape for l in m.layers] == [(84, 20, 32), (84, 9, 64), (84, 7, 64), (37632,),
                                               (512,), (12,)]


def test_create_model_for_other_agents_ignores_n_atoms():
    from xagents_amd.utils.common import create_model
    env = _env(obs=(84, 84, 1), n=6)
    a = create_model(env, 'dqn', 'model', seed=3, device='cpu')
    b = create_model(env, 'dqn', 'model', seed=3, device='cpu', n_atoms=7)
    for m in (a, b):
        assert m.layers[-1].units == 6
    np.testing.assert_array_equal(a.theta.numpy(), b.theta.numpy())
    m = create_model(_env(n=3), 'qrdqn', 'model', seed=1, device='cpu', n_atoms=7)
    assert m.layers[-1].units == 3 * 32
    m = create_model(_env(n=3), 'c51', 'model', seed=1, device='cpu', n_quantiles=7)
    assert m.layers[-1].units == 3 * 51


@pytest.mark.parametrize('kwargs,error,match', [
    (dict(huber_delta=1.0), TypeError, 'huber_delta'),
    (dict(n_atoms=1), ValueError, 'n_atoms'),
    (dict(n_atoms=257), ValueError, 'n_atoms'),
    (dict(v_min=1.0, v_max=1.0), ValueError, 'v_min < v_max'),
    (dict(v_min=2.0, v_max=-2.0), ValueError, 'v_min < v_max'),
    (dict(v_max=float('inf')), ValueError, 'v_min < v_max'),
    (dict(v_min=float('nan')), ValueError, 'v_min < v_max'),
])
def test_constructor_refuses_bad_arguments(kwargs, error, match):
    """Checked before anything is built, so no env or device is needed."""
    from xagents_amd import C51
    with pytest.raises(error, match=match):
        C51(None, None, None, **kwargs)


def test_entry_points_refuse_illegal_shapes_on_the_host():
    """K = 257, K = 1, A = 0 and a support that is not finite with v_max > v_min are refused
    before any device call (so this runs without a GPU) with a message naming the limit."""
    from xagents_amd import _lib
    lib = _lib.load()
    for name in ('xa_c51_act', 'xa_c51_project', 'xa_c51_td_grad'):
        assert name in _lib.EXPORTED_SYMBOLS
    p = 64  # any non-null address: nothing is launched
    inf, nan = float('inf'), float('nan')

    def td(A, K, lo, hi):
        return lib.xa_c51_td_grad(p, p, None, None, p, p, p, 4, A, K, lo, hi, 0.99, p, None,
                                  None, None, None, None, None)

    def project(A, K, lo, hi):
        return lib.xa_c51_project(p, None, p, p, None, 4, A, K, lo, hi, 0.99, p, None)

    def act(A, K, lo, hi):
        return lib.xa_c51_act(p, 4, A, K, lo, hi, None, 0, p, None, None)

    for fn in (td, project, act):
        assert fn(2, 257, -10.0, 10.0) != 0 and b'n_atoms <= 256' in lib.xa_last_error()
        assert fn(2, 1, -10.0, 10.0) != 0 and b'2 <= n_atoms' in lib.xa_last_error()
        assert fn(0, 8, -10.0, 10.0) != 0 and b'n_actions >= 1' in lib.xa_last_error()
        for lo, hi in ((1.0, 1.0), (2.0, -2.0), (-inf, 1.0), (0.0, inf), (nan, 1.0), (0.0, nan),
                       (-3e38, 3e38)):
            assert fn(2, 8, lo, hi) != 0 and b'v_max > v_min' in lib.xa_last_error()
    assert lib.xa_c51_td_grad(p, None, None, None, p, p, p, 4, 2, 8, -1.0, 1.0, 0.99, p, None,
                              None, None, None, None, None) != 0
    assert lib.xa_c51_act(None, 4, 2, 8, -1.0, 1.0, None, 0, p, None, None) != 0
