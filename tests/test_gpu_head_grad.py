"""xa_ac_head_grad called directly through the C ABI against the float64 restatement
(heads_ref.heads_terms_f64): d loss / d logits (or d Gaussian mean), d loss / d value and
the [pg, value, entropy] loss means, for both loss kinds and both distributions.

Bounds. The metric is max |got - ref| / max |ref| (as _assert_grad_close of
test_gpu_kernels.py), over dlogits and dvalues taken as one gradient vector and over the
three loss means. Measured on an MI355X with the kernels as they were before
ac_loss.hpp existed, the largest values over every case below were
    gradients  4.894e-07 (Gaussian 1025 x 3, PPO),   loss means  1.099e-07 (Categorical 1 x 2);
the bounds are four times those (the margin covers the seed-to-seed variation of f32
rounding in the 1/n-scaled sums), and the test passed on those kernels unchanged.

Shapes: n = 1025 sends the 1024-thread stride loop into a second pass, A = 64 is the
kernel's largest action count, n = 1 has zero advantage variance (its PPO policy gradient
is zero; the seeds keep its value gradient). Inputs are generated as
_rand_batch of test_gpu_kernels.py does: old log-prob noise 0.1 and old value noise 0.3
against clip 0.1 put samples on every side of both clips. The seeds are chosen so that
(test_reference_covers_every_branch, no GPU needed) the reference of every case with
n >= 63 has samples in all six branches of the PPO loss and none within 1e-5 of a branch
boundary, so no sample's branch depends on f32 rounding and none is left out of the
comparison."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch
from heads_ref import LOG2PI, heads_terms_f64

GRAD_TOL = 4 * 4.894e-07
LOSS_TOL = 4 * 1.099e-07
CLIP, ENT_COEF, V_COEF, EPS = 0.1, 0.01, 0.5, 1e-8
EDGE = 1e-5

# (dist, n, A or d, seed)
SHAPES = [('cat', 1, 2, 0), ('cat', 63, 3, 0), ('cat', 1025, 6, 3), ('cat', 130, 64, 4),
          ('gauss', 1, 1, 1), ('gauss', 1025, 3, 3)]
CASES = [s + (kind,) for s in SHAPES for kind in ('ppo', 'a2c')]
IDS = [f'{d}-{n}x{A}-{kind}' for d, n, A, _, kind in CASES]


@lru_cache(maxsize=None)
def _inputs(dist, n, A, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    z = rng.standard_normal((n, A)).astype(f)
    val = rng.standard_normal(n).astype(f)
    if dist == 'gauss':
        act = (z + rng.standard_normal((n, A))).astype(f)
        logp = -0.5 * ((act.astype(np.float64) - z) ** 2).sum(1) - 0.5 * A * LOG2PI
    else:
        act = rng.integers(0, A, n).astype(np.int32)
        z64 = z.astype(np.float64)
        m = z64.max(-1, keepdims=True)
        logp = (z64 - m - np.log(np.exp(z64 - m).sum(-1, keepdims=True)))[np.arange(n), act]
    old_logp = (logp + rng.normal(0, 0.1, n)).astype(f)
    old_val = (val + rng.normal(0, 0.3, n)).astype(f)
    ret = (old_val + rng.normal(0, 1.0, n)).astype(f)
    return dict(z=z, val=val, act=act, old_logp=old_logp, old_val=old_val, ret=ret)


@lru_cache(maxsize=None)
def _ref(dist, n, A, seed, kind):
    c = _inputs(dist, n, A, seed)
    return heads_terms_f64(c['z'], c['val'], c['act'], c['old_logp'], c['old_val'], c['ret'],
                           kind, 'gauss' if dist == 'gauss' else 'logits', clip=CLIP,
                           ent_coef=ENT_COEF, v_coef=V_COEF, eps=EPS)


def _branches(t):
    """Sample counts of the six PPO branches, and the smallest distance of any sample
    from a branch boundary. Inside a clip range both inputs of the maximum are the same
    number, so pg1 / pg2 and vl1 / vl2 are compared where the clip is active."""
    r_in, v_in = t['r_in'], t['v_in']
    first = t['pg1'] >= t['pg2']
    unclipped = t['vl1'] >= t['vl2']
    counts = dict(pg_first=int((first & ~r_in).sum()), pg_inside=int(r_in.sum()),
                  pg_zero=int((~first & ~r_in).sum()),
                  v_unclipped=int((unclipped & ~v_in).sum()), v_inside=int(v_in.sum()),
                  v_zero=int((~unclipped & ~v_in).sum()))
    edge = min(np.abs(t['ratio'] - (1 - CLIP)).min(), np.abs(t['ratio'] - (1 + CLIP)).min(),
               np.abs(t['dvo'] - CLIP).min(), np.abs(t['dvo'] + CLIP).min(),
               np.abs(t['pg1'] - t['pg2'])[~r_in].min(initial=np.inf),
               np.abs(t['vl1'] - t['vl2'])[~v_in].min(initial=np.inf))
    return counts, float(edge)


@pytest.mark.parametrize('dist,n,A,seed', [s for s in SHAPES if s[1] >= 63],
                         ids=[f'{s[0]}-{s[1]}x{s[2]}' for s in SHAPES if s[1] >= 63])
def test_reference_covers_every_branch(dist, n, A, seed):
    counts, edge = _branches(_ref(dist, n, A, seed, 'ppo'))
    assert min(counts.values()) >= 1, counts
    assert edge > EDGE, edge


def _T(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _head_grad(device, dist, n, A, seed, kind, stats_mode=0, stats=None, wide=False):
    """(dlogits [n, A], dvalues [n], loss [3]) of one xa_ac_head_grad call; wide: both
    heads come out of one [n, A + 2] row (logits first, the value in column A)."""
    from xagents_amd._lib import (XA_DIST_CATEGORICAL, XA_DIST_DIAG_GAUSSIAN, XA_LOSS_A2C,
                                  XA_LOSS_PPO, XaHeadGradArgs, call, stream)
    c = _inputs(dist, n, A, seed)
    if wide:
        row = np.full((n, A + 2), np.nan, np.float32)
        row[:, :A], row[:, A] = c['z'], c['val']
        heads = _T(row, device)
        logits_ptr, values_ptr, ld = heads.data_ptr(), heads.data_ptr() + 4 * A, A + 2
        ld_v = ld
    else:
        heads = (_T(c['z'], device), _T(c['val'], device))
        logits_ptr, values_ptr, ld, ld_v = heads[0].data_ptr(), heads[1].data_ptr(), A, 1
    act, old_logp, old_val, ret = (_T(c[k], device) for k in ('act', 'old_logp', 'old_val', 'ret'))
    dz = torch.full((n, A), float('nan'), device=device)
    dv = torch.full((n,), float('nan'), device=device)
    loss = torch.full((3,), float('nan'), device=device)
    h = XaHeadGradArgs()
    h.n, h.n_actions = n, A
    h.loss_kind = XA_LOSS_PPO if kind == 'ppo' else XA_LOSS_A2C
    h.logits, h.ld_logits, h.values, h.ld_values = logits_ptr, ld, values_ptr, ld_v
    if dist == 'gauss':
        h.dist_kind, h.actions_f, h.ld_actions = XA_DIST_DIAG_GAUSSIAN, act.data_ptr(), A
    else:
        h.dist_kind, h.actions = XA_DIST_CATEGORICAL, act.data_ptr()
    h.old_logp, h.old_values, h.returns = old_logp.data_ptr(), old_val.data_ptr(), ret.data_ptr()
    h.clip_norm, h.entropy_coef, h.value_coef, h.adv_eps = CLIP, ENT_COEF, V_COEF, EPS
    h.dlogits, h.dvalues, h.loss = dz.data_ptr(), dv.data_ptr(), loss.data_ptr()
    h.stats_mode = stats_mode
    h.adv_stats = None if stats is None else stats.data_ptr()
    call('xa_ac_head_grad', ctypes.byref(h), stream())
    torch.cuda.synchronize()
    return dz.cpu().numpy(), dv.cpu().numpy(), loss.cpu().numpy()


def _errors(got, t):
    """(gradient error, loss-mean error) of a (dlogits, dvalues, loss) triple"""
    dz, dv, loss = got
    g = np.concatenate([dz.ravel().astype(np.float64), dv.astype(np.float64)])
    g_ref = np.concatenate([t['dz'].ravel(), t['dv']])
    l_ref = np.array([t['pg'].mean(), t['vl'].mean(), t['ent'].mean()])
    return (np.abs(g - g_ref).max() / np.abs(g_ref).max(),
            np.abs(loss - l_ref).max() / np.abs(l_ref).max())


def _check(got, t, what):
    assert all(np.isfinite(x).all() for x in got), what
    g_err, l_err = _errors(got, t)
    print(f'{what}: gradient {g_err:.3e} loss means {l_err:.3e}')
    assert g_err < GRAD_TOL and l_err < LOSS_TOL, \
        f'{what}: gradient {g_err:.3e} (< {GRAD_TOL:.1e}) loss means {l_err:.3e} (< {LOSS_TOL:.1e})'


@pytest.mark.gpu
@pytest.mark.parametrize('dist,n,A,seed,kind', CASES, ids=IDS)
def test_head_grad_vs_f64(device, dist, n, A, seed, kind):
    _check(_head_grad(device, dist, n, A, seed, kind), _ref(dist, n, A, seed, kind),
           f'{dist} {n}x{A} {kind}')


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['ppo', 'a2c'])
def test_head_grad_heads_in_one_wider_row(device, kind):
    """ld_logits > A and ld_values > 1: the executor hands both heads out of one row."""
    dist, n, A, seed = SHAPES[1]
    _check(_head_grad(device, dist, n, A, seed, kind, wide=True), _ref(dist, n, A, seed, kind),
           f'wide row {kind}')


@pytest.mark.gpu
def test_head_grad_given_statistics_bit_exact(device):
    """stats_mode 1 writes [sum adv, sum adv^2, n] and nothing else; fed back with
    stats_mode 2 they give the bits of stats_mode 0."""
    dist, n, A, seed = SHAPES[2]
    own = _head_grad(device, dist, n, A, seed, 'ppo')
    stats = torch.zeros(3, dtype=torch.float64, device=device)
    wrote = _head_grad(device, dist, n, A, seed, 'ppo', stats_mode=1, stats=stats)
    assert all(np.isnan(x).all() for x in wrote)
    c = _inputs(dist, n, A, seed)
    adv = (c['ret'] - c['old_val']).astype(np.float64)
    s = stats.cpu().numpy()
    np.testing.assert_allclose(s[:2], [adv.sum(), (adv ** 2).sum()], rtol=1e-12)
    assert s[2] == n
    given = _head_grad(device, dist, n, A, seed, 'ppo', stats_mode=2, stats=stats)
    for a, b in zip(own, given):
        np.testing.assert_array_equal(a, b)
