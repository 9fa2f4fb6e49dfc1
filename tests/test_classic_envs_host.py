"""Acrobot-v1 / MountainCar-v0 device envs, host side (no GPU): the numpy f64 restatement of
the two gym dynamics that the GPU tests (tests/test_gpu_classic_envs.py) use as their
reference, checked on its own; the argument refusals of xa_classic_step / xa_mlp_rollout
(before any device call); the new entry point's registration; create_envs' modes.

The restatement is written from gym's formulas (classic_control/acrobot.py, "book" dynamics
with dt = 0.2 and classical RK4, and classic_control/mountain_car.py), vectorised over envs;
it shares no code with the product.
"""
import ctypes
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

ACROBOT, MOUNTAINCAR = 2, 3
OBS_DIM = {ACROBOT: 6, MOUNTAINCAR: 2}
TIME_LIMIT = {ACROBOT: 500, MOUNTAINCAR: 200}
NEAR = 1e-9  # a reference margin closer than this to a threshold: the branch is not compared


# ---- numpy f64 restatement ---------------------------------------------------------------
def acrobot_dsdt(s, tau):
    m1 = m2 = 1.0
    l1 = 1.0
    lc1 = lc2 = 0.5
    I1 = I2 = 1.0
    g = 9.8
    th1, th2, w1, w2 = s.T
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * np.cos(th2)) + I1 + I2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * np.cos(th2)) + I2
    phi2 = m2 * lc2 * g * np.cos(th1 + th2 - np.pi / 2.0)
    phi1 = (-m2 * l1 * lc2 * w2 ** 2 * np.sin(th2) - 2 * m2 * l1 * lc2 * w2 * w1 * np.sin(th2)
            + (m1 * lc1 + m2 * l1) * g * np.cos(th1 - np.pi / 2) + phi2)
    dd2 = (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 ** 2 * np.sin(th2) - phi2) / (
        m2 * lc2 ** 2 + I2 - d2 ** 2 / d1)
    dd1 = -(d2 * dd2 + phi1) / d1
    return np.stack([w1, w2, dd1, dd2], 1)


def _wrap(x):
    x = x.copy()
    while (x > np.pi).any():
        x = np.where(x > np.pi, x - 2 * np.pi, x)
    while (x < -np.pi).any():
        x = np.where(x < -np.pi, x + 2 * np.pi, x)
    return x


def acrobot_step(s, a):
    """One env.step of every row of s [n, 4] with actions a [n]: the new state, gym's
    `terminated`, the margins whose sign decides a done, and which branches fired."""
    tau = (a - 1).astype(np.float64)
    k1 = acrobot_dsdt(s, tau)
    k2 = acrobot_dsdt(s + 0.1 * k1, tau)
    k3 = acrobot_dsdt(s + 0.1 * k2, tau)
    k4 = acrobot_dsdt(s + 0.2 * k3, tau)
    y = s + 0.2 / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    ns = np.stack([_wrap(y[:, 0]), _wrap(y[:, 1]), np.clip(y[:, 2], -4 * np.pi, 4 * np.pi),
                   np.clip(y[:, 3], -9 * np.pi, 9 * np.pi)], 1)
    margin = -np.cos(ns[:, 0]) - np.cos(ns[:, 1] + ns[:, 0]) - 1.0
    events = dict(terminal=margin > 0, clip=(ns[:, 2] != y[:, 2]) | (ns[:, 3] != y[:, 3]),
                  wrap=(ns[:, 0] != y[:, 0]) | (ns[:, 1] != y[:, 1]))
    return ns, margin > 0, [margin], events


def mountaincar_step(s, a):
    p, v = s[:, 0], s[:, 1]
    v = v + ((a - 1) * 0.001 + np.cos(3 * p) * (-0.0025))
    v = np.clip(v, -0.07, 0.07)
    pu = p + v
    p = np.clip(pu, -1.2, 0.6)
    wall = (p == -1.2) & (v < 0)
    v_hit = v
    v = np.where(wall, 0.0, v)
    term = (p >= 0.5) & (v >= 0)
    ns = s.copy()
    ns[:, 0], ns[:, 1] = p, v
    # the goal line, the sign of the velocity, the (unclipped) position at the wall
    return ns, term, [p - 0.5, v_hit, pu + 1.2], dict(goal=term, wall=wall)


def observe(kind, s):
    if kind == ACROBOT:
        o = np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]),
                      s[:, 2], s[:, 3]], 1)
    else:
        o = s[:, :2]
    return o.astype(np.float32)


def ref_step(kind, s, elapsed, a, limit):
    """The record of one step of every env: pre-reset state and its f32 observation, reward,
    done (terminated or TimeLimit), `near` (a margin within NEAR of its threshold) and the
    branches that fired."""
    ns, term, margins, events = (acrobot_step if kind == ACROBOT else mountaincar_step)(s, a)
    el = elapsed + 1
    done = term | (el >= limit)
    rew = np.where(term, 0.0, -1.0) if kind == ACROBOT else np.full(len(s), -1.0)
    near = np.zeros(len(s), bool)
    for m in margins:
        near |= np.abs(m) < NEAR
    events = dict(events, timelimit=done & ~term)
    return dict(state=ns, obs=observe(kind, ns), rew=rew.astype(np.float32), done=done,
                elapsed=el, near=near, events=events)


def wide_start(kind, n, rng):
    """Starting states that reach every branch within a few steps. Acrobot: angles over the
    circle, velocities across their bounds (terminal, velocity clip, angle wrap).
    MountainCar: a third of the envs just below the goal moving right, a third next to the
    left wall moving left, the rest a gym reset."""
    s = np.zeros((n, 4))
    if kind == ACROBOT:
        s[:, :2] = rng.uniform(-np.pi, np.pi, (n, 2))
        s[:, 2] = rng.uniform(-4 * np.pi, 4 * np.pi, n)
        s[:, 3] = rng.uniform(-9 * np.pi, 9 * np.pi, n)
    else:
        s[:, 0] = rng.uniform(-0.6, -0.4, n)
        k = n // 3
        s[:k, 0], s[:k, 1] = rng.uniform(0.3, 0.5, k), 0.05
        s[k:2 * k, 0], s[k:2 * k, 1] = -1.19, -0.05
    return s


def reset_in_range(kind, s):
    if kind == ACROBOT:
        return (np.abs(s) <= 0.1).all(1)
    return (s[:, 0] >= -0.6) & (s[:, 0] <= -0.4) & (s[:, 1] == 0.0)


# the teacher-forced step test's case (tests/test_gpu_classic_envs.py (a)): 37 envs (not a
# multiple of the wave or the workgroup), 200 steps, Acrobot under a 20-step TimeLimit
STEP_CASE = dict(n=37, steps=200, seed=20261, limit={ACROBOT: 20, MOUNTAINCAR: 200})
STEP_EVENTS = {ACROBOT: ('terminal', 'clip', 'wrap', 'timelimit'),
               MOUNTAINCAR: ('goal', 'wall', 'timelimit')}


def step_case(kind):
    rng = np.random.default_rng(STEP_CASE['seed'] + kind)
    s0 = wide_start(kind, STEP_CASE['n'], rng)
    acts = rng.integers(0, 3, (STEP_CASE['steps'], STEP_CASE['n'])).astype(np.int32)
    return s0, acts


# ---- the restatement itself ----------------------------------------------------------------
def test_acrobot_rest_is_a_fixed_point():
    s = np.zeros((3, 4))
    assert np.abs(acrobot_dsdt(s, np.zeros(3))).max() < 1e-15
    ns, term, _, _ = acrobot_step(s, np.ones(3, np.int64))
    assert np.abs(ns).max() < 1e-14 and not term.any()
    # (cos(-pi / 2) is 6e-17 in f64, not 0: hence the bounds instead of equality.) Hanging
    # straight down the observation is (1, 0, 1, 0, 0, 0)
    assert np.array_equal(observe(ACROBOT, s), np.tile(np.float32([1, 0, 1, 0, 0, 0]), (3, 1)))
    assert np.abs(observe(ACROBOT, ns) - observe(ACROBOT, s)).max() < 1e-14


def test_mountaincar_coasting_step():
    s = np.array([[-0.5, 0.0, 0.0, 0.0]])
    ns, term, _, ev = mountaincar_step(s, np.array([1]))
    dv = np.cos(-1.5) * (-0.0025)
    assert ns[0, 1] == dv and ns[0, 0] == -0.5 + dv and not term[0] and not ev['wall'][0]
    # the wall stops the car dead; the goal needs a non-negative velocity
    ns, term, _, ev = mountaincar_step(np.array([[-1.19, -0.05, 0, 0], [0.49, 0.05, 0, 0]]),
                                       np.array([0, 2]))
    assert ev['wall'][0] and ns[0, 0] == -1.2 and ns[0, 1] == 0.0 and not term[0]
    assert term[1] and ns[1, 0] >= 0.5


@pytest.mark.parametrize('kind', [ACROBOT, MOUNTAINCAR])
def test_step_case_reaches_every_branch_away_from_the_thresholds(kind):
    """The reference alone, on the GPU step test's start states and actions (resets from a
    numpy generator): every branch fires, and no sample sits within NEAR of a threshold, so
    whatever the GPU test excludes comes from the device's own trajectory."""
    s, acts = step_case(kind)
    rng = np.random.default_rng(1)
    limit = STEP_CASE['limit'][kind]
    el = np.zeros(len(s), np.int64)
    seen = {k: 0 for k in STEP_EVENTS[kind]}
    for a in acts:
        r = ref_step(kind, s, el, a, limit)
        assert not r['near'].any()
        for k in seen:
            seen[k] += int(r['events'][k].sum())
        fresh = np.zeros_like(s)
        if kind == ACROBOT:
            fresh[:] = rng.uniform(-0.1, 0.1, s.shape)
        else:
            fresh[:, 0] = rng.uniform(-0.6, -0.4, len(s))
        assert reset_in_range(kind, fresh).all()
        s = np.where(r['done'][:, None], fresh, r['state'])
        el = np.where(r['done'], 0, r['elapsed'])
    assert all(v > 0 for v in seen.values()), seen


# ---- C ABI ---------------------------------------------------------------------------------
def test_classic_step_is_registered():
    from xagents_amd import _lib
    header = (ROOT / 'include' / 'xagents_hip.h').read_text()
    assert 'int xa_classic_step(const XaClassicStepArgs* args, void* stream);' in header
    assert 'xa_classic_step' in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.load(), 'xa_classic_step')
    assert f'#define XA_ENV_ACROBOT {_lib.XA_ENV_ACROBOT}' in header and _lib.XA_ENV_ACROBOT == 2
    assert f'#define XA_ENV_MOUNTAINCAR {_lib.XA_ENV_MOUNTAINCAR}' in header
    assert _lib.XA_ENV_MOUNTAINCAR == 3
    assert 'xa_classic_step' in (ROOT / 'INTEGRATION.md').read_text()
    assert _lib.load().xa_abi_version() == 2


def test_classic_step_refuses_bad_arguments():
    """Checked on the host before any device call (so this runs without a GPU)."""
    from xagents_amd import _lib
    lib = _lib.load()
    mem = (ctypes.c_double * 64)()  # never dereferenced: every call below is refused
    p = ctypes.addressof(mem)

    def args():
        a = _lib.XaClassicStepArgs()
        a.env_kind, a.n_envs = ACROBOT, 4
        a.state64 = a.elapsed = a.actions = a.out_obs = a.out_post = a.out_rew = a.out_done = p
        a.act_ld, a.max_episode_steps = 1, 500
        return a

    a = args()
    a.state64 = None
    assert lib.xa_classic_step(ctypes.byref(a), None) != 0
    assert b'state64' in lib.xa_last_error()
    for limit in (0, -3):
        a = args()
        a.max_episode_steps = limit
        assert lib.xa_classic_step(ctypes.byref(a), None) != 0
        assert b'max_episode_steps' in lib.xa_last_error()
    a = args()
    a.env_kind = 1  # CartPole has no step kernel
    assert lib.xa_classic_step(ctypes.byref(a), None) != 0
    assert b'env_kind' in lib.xa_last_error()
    a = args()
    a.actions = None
    assert lib.xa_classic_step(ctypes.byref(a), None) != 0
    assert b'actions' in lib.xa_last_error()


def test_rollout_refuses_bad_classic_env_arguments():
    from xagents_amd import _lib
    lib = _lib.load()
    mem = (ctypes.c_double * 64)()  # never dereferenced: every call below is refused
    p = ctypes.addressof(mem)

    def args(kind, obs, actions):
        a = _lib.XaRolloutArgs()
        a.n_envs, a.n_steps, a.obs_dim, a.n_actions = 4, 8, obs, actions
        a.env_kind = kind
        for name in ('theta', 'env_state', 'env_state64', 'env_done', 'env_cursor', 'ep_return',
                     'obs_out', 'act_out', 'logp_out', 'val_out', 'rew_out', 'done_out',
                     'next_val', 'rng_counter'):
            setattr(a, name, p)
        a.max_episode_steps = 500
        return a

    for kind, obs in ((ACROBOT, 6), (MOUNTAINCAR, 2)):
        a = args(kind, obs, 3)
        a.env_state64 = None
        assert lib.xa_mlp_rollout(ctypes.byref(a), None) != 0
        assert b'env_state64' in lib.xa_last_error()
        a = args(kind, obs, 3)
        a.max_episode_steps = 0
        assert lib.xa_mlp_rollout(ctypes.byref(a), None) != 0
        assert b'max_episode_steps' in lib.xa_last_error()
    # a kind and a shape that disagree
    for kind, obs, actions in ((ACROBOT, 4, 2), (ACROBOT, 2, 3), (MOUNTAINCAR, 6, 3)):
        a = args(kind, obs, actions)
        assert lib.xa_mlp_rollout(ctypes.byref(a), None) != 0
        assert b'needs obs_dim' in lib.xa_last_error()
    a = args(4, 6, 3)
    assert lib.xa_mlp_rollout(ctypes.byref(a), None) != 0
    assert b'unknown env_kind' in lib.xa_last_error()


def test_create_envs_modes_of_the_classic_ids():
    """An explicit 'replay' for the new ids names the two modes that exist (raised before
    any device allocation); every other id keeps 'replay' as its default."""
    import inspect
    from xagents_amd.envs import create_envs
    for env_id in ('Acrobot-v1', 'MountainCar-v0'):
        with pytest.raises(ValueError, match="'dynamics'.*'transitions'"):
            create_envs(env_id, 2, mode='replay')
    assert inspect.signature(create_envs).parameters['mode'].default is None
    with pytest.raises(NotImplementedError):
        create_envs('LunarLander-v2', 2)
