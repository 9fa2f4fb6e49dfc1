"""Pendulum-v1 / MountainCarContinuous-v0 device envs, host side (no GPU): the numpy f64
restatement of the two dynamics that the GPU tests (tests/test_gpu_continuous_envs.py) use as
their reference, checked on its own against hand-computed steps; the argument refusals of
xa_continuous_env_step (before any device call); the entry point's registration;
create_envs' modes.

The restatement is written from the formulas of gym's classic_control/pendulum.py and
continuous_mountain_car.py as DESIGN.md section 4 states them (gym itself is not part of the
build), vectorised over envs; it shares no code with the product.
"""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

PENDULUM, MOUNTAINCAR_CONT = 4, 5
KINDS = [PENDULUM, MOUNTAINCAR_CONT]
ENV_ID = {PENDULUM: 'Pendulum-v1', MOUNTAINCAR_CONT: 'MountainCarContinuous-v0'}
OBS_DIM = {PENDULUM: 3, MOUNTAINCAR_CONT: 2}
TIME_LIMIT = {PENDULUM: 200, MOUNTAINCAR_CONT: 999}
ACTION_BOUND = {PENDULUM: 2.0, MOUNTAINCAR_CONT: 1.0}
NEAR = 1e-9  # a reference margin closer than this to a threshold: the branch is not compared


# ---- numpy f64 restatement ---------------------------------------------------------------
def norm(x):
    """gym's angle_normalize; numpy's % on floats is Python's floor modulo."""
    return (x + np.pi) % (2 * np.pi) - np.pi


def pendulum_step(s, a):
    """One env.step of every row of s [n, 2] with raw actions a [n] (f64): the new state,
    the f64 reward, and which branches fired."""
    g, m, l, dt = 10.0, 1.0, 1.0, 0.05
    th, thdot = s.T
    u = np.minimum(np.maximum(a, -2.0), 2.0)
    cost = norm(th) ** 2 + 0.1 * thdot ** 2 + 0.001 * u ** 2
    raw = thdot + (3 * g / (2 * l) * np.sin(th) + 3.0 / (m * l ** 2) * u) * dt
    nthdot = np.minimum(np.maximum(raw, -8.0), 8.0)
    nth = th + nthdot * dt
    events = dict(torque_lo=a < -2.0, torque_hi=a > 2.0, speed_lo=raw < -8.0,
                  speed_hi=raw > 8.0, norm_wrap=np.abs(th) > np.pi)
    return np.stack([nth, nthdot], 1), -cost, events


def mountaincar_cont_step(s, a):
    """As pendulum_step, plus gym's `terminated` and the samples whose branch margins lie
    within NEAR of a threshold (goal line, velocity sign, wall)."""
    x, v = s.T
    f = np.minimum(np.maximum(a, -1.0), 1.0)
    raw_v = v + (f * 0.0015 - 0.0025 * np.cos(3 * x))
    v = np.minimum(np.maximum(raw_v, -0.07), 0.07)
    raw_x = x + v
    x = np.minimum(np.maximum(raw_x, -1.2), 0.6)
    wall = (x == -1.2) & (v < 0)
    v = np.where(wall, 0.0, v)
    terminated = (x >= 0.45) & (v >= 0)
    reward = np.where(terminated, 100.0, 0.0) - 0.1 * a ** 2
    near = (np.abs(raw_x + 1.2) < NEAR) | ((x == -1.2) & (np.abs(v) < NEAR) & ~wall) \
        | ((np.abs(x - 0.45) < NEAR) & (v >= -NEAR)) | ((x >= 0.45 - NEAR) & (np.abs(v) < NEAR))
    events = dict(force_lo=a < -1.0, force_hi=a > 1.0, speed_lo=raw_v < -0.07,
                  speed_hi=raw_v > 0.07, wall=wall, goal=terminated)
    return np.stack([x, v], 1), reward, terminated, near, events


STEP_EVENTS = {PENDULUM: ('torque_lo', 'torque_hi', 'speed_lo', 'speed_hi', 'norm_wrap',
                          'time_limit'),
               MOUNTAINCAR_CONT: ('force_lo', 'force_hi', 'speed_lo', 'speed_hi', 'wall', 'goal',
                                  'time_limit')}


def observe(kind, s):
    """The f32 observation of f64 states s [n, 2]."""
    if kind == PENDULUM:
        return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), s[:, 1]], 1).astype(np.float32)
    return s.astype(np.float32)


def reset_in_range(kind, s):
    if kind == PENDULUM:
        return (np.abs(s[:, 0]) <= np.pi) & (np.abs(s[:, 1]) <= 1.0)
    return (s[:, 0] >= -0.6) & (s[:, 0] <= -0.4) & (s[:, 1] == 0.0)


def ref_step(kind, s, elapsed, a, limit):
    """One step of every (state [m, 2] f64, elapsed [m], raw f32 action [m]) sample: the
    stepped f64 state (pre-reset), its f32 observation, the f32 reward, done (terminated or
    the TimeLimit), the new elapsed count (where the episode goes on), near, events."""
    a = a.astype(np.float32).astype(np.float64)  # the env reads f32 actions
    if kind == PENDULUM:
        ns, rew, events = pendulum_step(s, a)
        terminated = np.zeros(len(s), bool)
        near = np.zeros(len(s), bool)
    else:
        ns, rew, terminated, near, events = mountaincar_cont_step(s, a)
    el = elapsed + 1
    events = dict(events, time_limit=~terminated & (el >= limit))
    return dict(state=ns, obs=observe(kind, ns), rew=rew.astype(np.float32),
                done=terminated | (el >= limit), elapsed=el, near=near, events=events)


# ---- the step case of the GPU test: random actions beyond the action bounds, a short
# TimeLimit, and states planted by hand so that every branch is reached at every n_envs ------
STEP_CASE = dict(steps=200, limit=7, n_envs=(3, 257), act_ld=(1, 4))

# (state, raw action): what the sample must reach is in the comment
PLANTS = {
    PENDULUM: [((7.0, 7.9), 5.0),        # |th| > pi, torque clip high, speed clip high
               ((-7.0, -7.9), -5.0),     # torque clip low, speed clip low
               ((math.pi / 2, 7.99), 0.5),    # speed clip high without a torque clip
               ((-math.pi / 2, -7.99), -0.5)],
    MOUNTAINCAR_CONT: [((-1.19, -0.07), -1.7),  # left wall: x clipped to -1.2, v zeroed
                       ((0.0, -0.069), -1.7),   # force clip low, speed clip low
                       ((-0.5, 0.0695), 1.7),   # force clip high, speed clip high
                       ((0.44, 0.069), 1.7)],   # goal: reward 100 - 0.1 * 1.7^2
}


def step_case(kind, n):
    """actions [T, n] f32 and the plant schedule [(step, env, state, action)]: plant k goes
    to env k % n before step 10 * (k // n) + k % 2 (so small n_envs get them all too)."""
    T = STEP_CASE['steps']
    rng = np.random.default_rng(100 * kind + n)
    bound = ACTION_BOUND[kind]
    acts = rng.uniform(-1.6 * bound, 1.6 * bound, (T, n)).astype(np.float32)
    plants = []
    for k, (state, action) in enumerate(PLANTS[kind]):
        t, env = 10 * (k // n) + k % 2, k % n
        acts[t, env] = action
        plants.append((t, env, np.array(state), action))
    return acts, plants


def run_case_on_host(kind, n):
    """The step case run by the restatement alone (resets drawn by numpy inside gym's
    ranges): the event counts, and the reward of the planted goal sample."""
    T, limit = STEP_CASE['steps'], STEP_CASE['limit']
    acts, plants = step_case(kind, n)
    rng = np.random.default_rng(7)

    def draw(m):
        if kind == PENDULUM:
            return np.stack([rng.uniform(-np.pi, np.pi, m), rng.uniform(-1, 1, m)], 1)
        return np.stack([rng.uniform(-0.6, -0.4, m), np.zeros(m)], 1)

    s, el = draw(n), np.zeros(n, np.int64)
    seen = {name: 0 for name in STEP_EVENTS[kind]}
    near = 0
    for t in range(T):
        for pt, env, state, _ in plants:
            if pt == t:
                s[env] = state
        r = ref_step(kind, s, el, acts[t], limit)
        for name in seen:
            seen[name] += int(r['events'][name].sum())
        near += int(r['near'].sum())
        s = np.where(r['done'][:, None], draw(n), r['state'])
        el = np.where(r['done'], 0, r['elapsed'])
    return seen, near


# ---- the restatement on its own ------------------------------------------------------------
def test_norm_is_pythons_floor_modulo():
    eps = 1e-12
    xs = [math.pi, -math.pi, 3 * math.pi, -3 * math.pi]
    xs += [x + d for x in list(xs) for d in (eps, -eps)] + [0.0, 7.0, -7.0, 100.0]
    got = norm(np.array(xs))
    for x, y in zip(xs, got):
        want = (x + math.pi) % (2 * math.pi) - math.pi  # Python's own float %
        assert y == want, (x, y, want)
        assert -math.pi <= y < math.pi
    # the wrap itself: pi maps to -pi, just below pi stays, 7 rad is 7 - 2 pi
    assert norm(np.array([math.pi]))[0] == -math.pi
    assert norm(np.array([math.pi - eps]))[0] == pytest.approx(math.pi - eps, abs=1e-15)
    assert norm(np.array([-math.pi - eps]))[0] == pytest.approx(math.pi - eps, abs=1e-14)
    assert norm(np.array([7.0]))[0] == pytest.approx(7.0 - 2 * math.pi, abs=1e-15)


def test_pendulum_restatement_hand_computed_steps():
    # (th, thdot) = (pi / 2, 0), a = 5: u = 2, thdot' = 0.05 (15 sin(pi/2) + 3 * 2), the cost
    # from the pre-step state
    s, rew, ev = pendulum_step(np.array([[math.pi / 2, 0.0]]), np.array([5.0]))
    thdot = 0.05 * (15.0 + 6.0)
    assert s[0, 1] == pytest.approx(thdot, abs=1e-15)
    assert s[0, 0] == pytest.approx(math.pi / 2 + 0.05 * thdot, abs=1e-15)
    assert rew[0] == pytest.approx(-((math.pi / 2) ** 2 + 0.001 * 4.0), abs=1e-15)
    assert ev['torque_hi'][0] and not ev['torque_lo'][0] and not ev['speed_hi'][0]
    # the speed clip comes before the angle update; th is not wrapped in the state
    s, rew, ev = pendulum_step(np.array([[7.0, 7.9]]), np.array([-0.5]))
    raw = 7.9 + (15.0 * math.sin(7.0) - 1.5) * 0.05
    assert raw > 8.0 and ev['speed_hi'][0] and ev['norm_wrap'][0]
    assert s[0, 1] == 8.0 and s[0, 0] == pytest.approx(7.0 + 0.4, abs=1e-15) and s[0, 0] > math.pi
    cost = (7.0 - 2 * math.pi) ** 2 + 0.1 * 7.9 ** 2 + 0.001 * 0.25
    assert rew[0] == pytest.approx(-cost, abs=1e-13)
    s, _, ev = pendulum_step(np.array([[-math.pi / 2, -7.99]]), np.array([-3.0]))
    assert s[0, 1] == -8.0 and ev['speed_lo'][0] and ev['torque_lo'][0]
    obs = observe(PENDULUM, np.array([[math.pi / 3, -2.5]]))
    assert obs.dtype == np.float32
    assert obs[0] == pytest.approx([0.5, math.sqrt(3) / 2, -2.5], abs=1e-7)


def test_mountaincar_cont_restatement_hand_computed_steps():
    # the left wall: x clipped to -1.2 with v < 0 gives v = 0
    s, rew, term, near, ev = mountaincar_cont_step(np.array([[-1.2, -0.01]]), np.array([-1.0]))
    assert s[0, 0] == -1.2 and s[0, 1] == 0.0 and ev['wall'][0] and not term[0]
    assert rew[0] == pytest.approx(-0.1, abs=1e-15)
    # a = 1.7: the force is clipped to 1, the penalty uses the raw action (0.289)
    s, rew, term, near, ev = mountaincar_cont_step(np.array([[-0.5, 0.0]]), np.array([1.7]))
    v = 1.0 * 0.0015 - 0.0025 * math.cos(-1.5)
    assert ev['force_hi'][0] and s[0, 1] == pytest.approx(v, abs=1e-18)
    assert s[0, 0] == pytest.approx(-0.5 + v, abs=1e-15)
    assert rew[0] == pytest.approx(-0.289, abs=1e-15) and not term[0]
    # the goal: x >= 0.45 with v >= 0 terminates with 100 - 0.1 a^2
    s, rew, term, near, ev = mountaincar_cont_step(np.array([[0.44, 0.069]]), np.array([1.7]))
    assert term[0] and ev['goal'][0] and s[0, 0] >= 0.45 and not ev['speed_hi'][0]
    assert rew[0] == pytest.approx(100.0 - 0.289, abs=1e-13)
    # ... and not when moving left
    _, rew, term, _, _ = mountaincar_cont_step(np.array([[0.5, -0.03]]), np.array([0.0]))
    assert not term[0] and rew[0] == 0.0
    # speed clips on both sides, the right wall
    s, _, _, _, ev = mountaincar_cont_step(np.array([[0.0, -0.069]]), np.array([-1.7]))
    assert s[0, 1] == -0.07 and ev['speed_lo'][0] and ev['force_lo'][0]
    s, _, _, _, ev = mountaincar_cont_step(np.array([[-0.5, 0.0695]]), np.array([1.7]))
    assert s[0, 1] == 0.07 and ev['speed_hi'][0]
    s, _, term, _, _ = mountaincar_cont_step(np.array([[0.59, 0.07]]), np.array([1.0]))
    assert s[0, 0] == 0.6 and term[0]


def test_ref_step_applies_the_time_limit_and_f32_rounding():
    s = np.array([[0.3, 0.2], [0.3, 0.2]])
    r = ref_step(PENDULUM, s, np.array([5, 6]), np.array([0.1, 0.1], np.float32), 7)
    assert list(r['done']) == [False, True] and list(r['events']['time_limit']) == [False, True]
    assert list(r['elapsed']) == [6, 7]
    assert r['obs'].dtype == np.float32 and r['rew'].dtype == np.float32
    # the env reads the action as f32: 0.1f, not 0.1
    a = float(np.float32(0.1))
    _, rew, _ = pendulum_step(s[:1], np.array([a]))
    assert r['rew'][0] == np.float32(rew[0])


@pytest.mark.parametrize('n', STEP_CASE['n_envs'])
@pytest.mark.parametrize('kind', KINDS)
def test_step_case_reaches_every_branch(kind, n):
    """The inputs of the GPU test do reach every branch, at both env counts; the planted
    samples alone reach all but the TimeLimit whatever the resets are."""
    seen, near = run_case_on_host(kind, n)
    assert all(v > 0 for v in seen.values()), seen
    assert near == 0
    _, plants = step_case(kind, n)
    assert len({(t, env) for t, env, _, _ in plants}) == len(plants)  # no plant overwritten
    states = np.stack([p[2] for p in plants])
    acts = np.array([p[3] for p in plants], np.float32)
    r = ref_step(kind, states, np.zeros(len(plants), np.int64), acts, STEP_CASE['limit'])
    for name in STEP_EVENTS[kind]:
        if name != 'time_limit':
            assert r['events'][name].any(), name
    assert not r['near'].any()
    if kind == MOUNTAINCAR_CONT:
        goal = r['events']['goal']
        assert (r['rew'][goal] == np.float32(100.0 - 0.1 * np.float64(np.float32(1.7)) ** 2)).all()


# ---- C ABI ---------------------------------------------------------------------------------
def test_continuous_env_step_is_registered():
    from xagents_amd import _lib
    header = (ROOT / 'include' / 'xagents_hip.h').read_text()
    flat = re.sub(r'\s+', ' ', header)
    assert ('int xa_continuous_env_step(const XaContinuousStepArgs* env, '
            'const XaReplayStepArgs* step, void* stream);') in flat
    assert 'xa_continuous_env_step' in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.load(), 'xa_continuous_env_step')
    assert f'#define XA_ENV_PENDULUM {_lib.XA_ENV_PENDULUM}' in header and _lib.XA_ENV_PENDULUM == 4
    assert f'#define XA_ENV_MOUNTAINCAR_CONT {_lib.XA_ENV_MOUNTAINCAR_CONT}' in header
    assert _lib.XA_ENV_MOUNTAINCAR_CONT == 5
    assert 'xa_continuous_env_step' in (ROOT / 'INTEGRATION.md').read_text()
    assert _lib.load().xa_abi_version() == 2
    # the ctypes mirror has the header's fields, in order
    body = re.search(r'typedef struct XaContinuousStepArgs \{(.*?)\} XaContinuousStepArgs;',
                     header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in body.split(';') for n in re.findall(r'(\w+)\s*(?:,|$)', decl.strip())]
    assert names == [f[0] for f in _lib.XaContinuousStepArgs._fields_]


def _env_args(_lib, p, kind=PENDULUM):
    a = _lib.XaContinuousStepArgs()
    a.env_kind, a.n_envs = kind, 4
    a.state64 = a.elapsed = a.episode = a.actions = p
    a.out_obs = a.out_post = a.out_rew = a.out_done = p
    a.act_ld, a.max_episode_steps = 1, 200
    return a


def _step_args(_lib, p, kind=PENDULUM, ring=True):
    r = _lib.XaReplayStepArgs()
    r.n_envs, r.obs_bytes = 4, 4 * OBS_DIM[kind]
    r.state = r.ep_return = r.done = p
    if ring:
        r.ring_states = r.ring_new_states = r.ring_actions = r.ring_rewards = p
        r.ring_dones = r.ring_count = r.actions = p
        r.capacity, r.act_bytes = 8, 4
    return r


def test_continuous_env_step_refuses_bad_arguments():
    """Every refusal is made on the host before any device call (so this runs without a
    GPU) and names the field."""
    from xagents_amd import _lib
    lib = _lib.load()
    mem = (ctypes.c_double * 64)()  # never dereferenced: every call below is refused
    p = ctypes.addressof(mem)

    def refused(a, r, field):
        ret = lib.xa_continuous_env_step(ctypes.byref(a) if a is not None else None,
                                         ctypes.byref(r) if r is not None else None, None)
        assert ret != 0, field
        assert field in lib.xa_last_error(), (field, lib.xa_last_error())

    refused(None, None, b'null env args')
    for kind in (0, 1, 2, 3, 6, -1):
        refused(_env_args(_lib, p, kind), None, b'env_kind')
    for n in (0, -2):
        a = _env_args(_lib, p)
        a.n_envs = n
        refused(a, None, b'n_envs')
    for field in ('state64', 'elapsed', 'episode'):
        for r in (None, _step_args(_lib, p)):
            a = _env_args(_lib, p)
            setattr(a, field, None)
            refused(a, r, field.encode())
    for limit in (0, -3):
        a = _env_args(_lib, p)
        a.max_episode_steps = limit
        refused(a, None, b'max_episode_steps')
    for r in (None, _step_args(_lib, p)):
        a = _env_args(_lib, p)
        a.actions = None
        refused(a, r, b'actions')
        for ld in (0, -1):
            a = _env_args(_lib, p)
            a.act_ld = ld
            refused(a, r, b'act_ld')
    # step == NULL: the record outputs (out_post alone for a reset)
    for field in ('out_obs', 'out_post', 'out_rew', 'out_done'):
        a = _env_args(_lib, p)
        setattr(a, field, None)
        refused(a, None, field.encode())
    a = _env_args(_lib, p)
    a.reset_only, a.out_post = 1, None
    refused(a, None, b'out_post')
    # step given
    for kind in KINDS:
        r = _step_args(_lib, p, kind)
        r.obs_bytes = 4 * OBS_DIM[kind] + 4
        refused(_env_args(_lib, p, kind), r, b'obs_bytes')
        r.obs_bytes = 0
        refused(_env_args(_lib, p, kind), r, b'obs_bytes')
    for field in ('state', 'ep_return', 'done'):
        r = _step_args(_lib, p)
        setattr(r, field, None)
        refused(_env_args(_lib, p), r, b'null step ' + field.encode())
    for field in ('ring_new_states', 'ring_actions', 'ring_rewards', 'ring_dones', 'ring_count',
                  'actions'):
        r = _step_args(_lib, p)
        setattr(r, field, None)
        refused(_env_args(_lib, p), r, b'incomplete replay ring')
    for name, value in (('capacity', 0), ('act_bytes', 0)):
        r = _step_args(_lib, p)
        setattr(r, name, value)
        refused(_env_args(_lib, p), r, b'incomplete replay ring')
    r = _step_args(_lib, p)
    r.n_envs = 5
    refused(_env_args(_lib, p), r, b'n_envs')
    a = _env_args(_lib, p)
    a.reset_only = 1
    refused(a, _step_args(_lib, p), b'reset_only')


def test_other_entry_points_keep_refusing_the_continuous_kinds():
    from xagents_amd import _lib
    lib = _lib.load()
    mem = (ctypes.c_double * 64)()
    p = ctypes.addressof(mem)
    for kind in KINDS:
        a = _lib.XaClassicStepArgs()
        a.env_kind, a.n_envs = kind, 4
        a.state64 = a.elapsed = a.actions = a.out_obs = a.out_post = a.out_rew = a.out_done = p
        a.act_ld, a.max_episode_steps = 1, 200
        assert lib.xa_classic_step(ctypes.byref(a), None) != 0
        assert b'env_kind' in lib.xa_last_error()
        ro = _lib.XaRolloutArgs()
        ro.n_envs, ro.n_steps, ro.obs_dim, ro.n_actions = 4, 8, OBS_DIM[kind], 3
        ro.env_kind = kind
        for name in ('theta', 'env_state', 'env_state64', 'env_done', 'env_cursor', 'ep_return',
                     'obs_out', 'act_out', 'logp_out', 'val_out', 'rew_out', 'done_out',
                     'next_val', 'rng_counter'):
            setattr(ro, name, p)
        ro.max_episode_steps = 200
        assert lib.xa_mlp_rollout(ctypes.byref(ro), None) != 0
        assert b'unknown env_kind' in lib.xa_last_error()


def test_create_envs_modes_of_the_continuous_ids():
    """The mode and option errors are raised before any device allocation (no GPU here);
    every other id behaves as before."""
    from xagents_amd.envs import CONTINUOUS_ENVS, ContinuousControlVecEnv, create_envs
    assert set(CONTINUOUS_ENVS) == set(ENV_ID.values())
    for kind, env_id in ENV_ID.items():
        assert CONTINUOUS_ENVS[env_id] == (kind, OBS_DIM[kind], ACTION_BOUND[kind],
                                           TIME_LIMIT[kind])
        with pytest.raises(ValueError, match="'dynamics'.*'transitions'"):
            create_envs(env_id, 2, mode='replay')
        with pytest.raises(AssertionError, match='non-atari'):
            create_envs(env_id, 2, preprocess=True)
        with pytest.raises(ValueError, match='max_episode_steps'):
            ContinuousControlVecEnv(env_id, 2, max_episode_steps=0)
    with pytest.raises(NotImplementedError):
        create_envs('LunarLander-v2', 2)
