"""Host checks of prioritized replay: the float64 restatement (tests/per_ref.py) against brute
force on the flat cumulative sum, the weights' normalisation, the draw's proportions, the
margins of every fixed input the GPU tests compare slots on, the tree shape on both sides of
the C ABI, the new entry points' declarations and the constructors that refuse the option."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import per_ref as R

ROOT = Path(__file__).resolve().parents[1]
PER_SYMBOLS = ('xa_per_rebuild', 'xa_per_mark', 'xa_per_sample', 'xa_per_update',
               'xa_dqn_td_grad_w', 'xa_sac_td_grad_w')
MARGIN = 1e-9


def _u24(rng, n):
    return (rng.integers(0, 1 << 24, n).astype(np.float64) * 2.0 ** -24).astype(np.float32)


@pytest.mark.parametrize('L', [1, 63, 64, 65, 70, 4096, 4097, 5000])
def test_descent_equals_brute_force(L):
    """np.searchsorted on the flat cumulative sum finds the same leaves (samples whose margin
    is above rounding, which all of these are), and never a zero leaf."""
    rng = np.random.default_rng(L)
    leaves = (rng.uniform(0.01, 2.0, L) * (rng.random(L) < 0.5)).astype(np.float32)
    leaves[rng.integers(L)] = 1.5
    for B in (1, 7, 64):
        u = _u24(rng, B)
        slots, margin = R.sample(leaves, u)
        assert margin.min() >= MARGIN
        np.testing.assert_array_equal(slots, R.sample_brute(leaves, u))
        assert (leaves[slots] > 0).all()


def test_tree_levels_and_sums():
    for L, want in ((1, [1]), (64, [1]), (65, [2, 1]), (70, [2, 1]), (4096, [64, 1]),
                    (4097, [65, 2, 1]), (64 ** 3, [4096, 64, 1]), (10 ** 6, [15625, 245, 4, 1])):
        assert R.level_sizes(L) == want
    leaves = np.arange(1, 71, dtype=np.float64)
    levels = R.build(leaves)
    np.testing.assert_array_equal(levels[0], [leaves[:64].sum(), leaves[64:].sum()])
    assert levels[1][0] == leaves.sum() and len(R.flat(levels)) == 3


def test_weights_are_batch_max_normalised_and_decreasing():
    rng = np.random.default_rng(2)
    leaf_p = rng.uniform(0.01, 2.0, 50)
    for beta in (0.4, 1.0):
        w = R.weights(leaf_p, root=37.0, n_stored=123, beta=beta)
        assert w.max() == 1.0 and w[np.argmin(leaf_p)] == 1.0
        order = np.argsort(leaf_p)
        assert (np.diff(w[order]) < 0).all()
    np.testing.assert_array_equal(R.weights(leaf_p, 37.0, 123, 0.0), np.ones(50))
    # beta = 1 undoes the sampling probability: w_j leaf_j is constant
    w = R.weights(leaf_p, 37.0, 123, 1.0)
    np.testing.assert_allclose(w * leaf_p, (w * leaf_p)[0], rtol=1e-12)


def test_hit_counts_follow_the_priorities():
    """400 batches of 64 on a 4097-leaf tree with 8 non-zero leaves: each leaf's count within 5
    standard deviations of B draws p_i / sum p (the binomial deviation: stratification only
    lowers it)."""
    rng = np.random.default_rng(5)
    L, B, draws = 4097, 64, 400
    leaves = np.zeros(L, np.float32)
    where = np.array([0, 63, 64, 1000, 2048, 4032, 4095, 4096])
    leaves[where] = rng.uniform(0.1, 3.0, 8).astype(np.float32)
    hits = np.zeros(L, np.int64)
    for _ in range(draws):
        slots, _ = R.sample(leaves, _u24(rng, B))
        np.add.at(hits, slots, 1)
    assert hits.sum() == B * draws and not hits[leaves == 0].any()
    p = leaves[where].astype(np.float64) / leaves.astype(np.float64).sum()
    n = B * draws
    sd = np.sqrt(n * p * (1 - p))
    assert (np.abs(hits[where] - n * p) <= 5 * sd).all(), (hits[where], n * p, sd)


@pytest.mark.parametrize('n_envs,cap', R.SHAPES)
def test_gpu_test_inputs_keep_their_margin(n_envs, cap):
    """Every fixed (leaves, uniforms) pair tests/test_gpu_per.py compares slots on."""
    leaves = R.case_leaves(n_envs, cap)
    for B in R.BATCHES:
        for flip in (False, True):
            u = R.case_uniforms(n_envs, cap, B, flip)
            assert {u[0], u[-1]} <= {R.U_LO, R.U_HI} and (u < 1).all()
            slots, margin = R.sample(leaves, u)
            assert margin.min() >= MARGIN, (B, flip, margin.min())
            assert (leaves[slots] > 0).all()


def test_mark_and_update_restatement():
    count = np.array([0, 3, 5, 12])
    np.testing.assert_array_equal(R.mark_slots(count, 5), [0, 8, 10, 17])
    assert R.stored(count, 5) == 0 + 3 + 5 + 5
    leaves = R.mark(np.zeros(20, np.float32), count, 5, 2.0, 0.6)
    assert np.count_nonzero(leaves) == 4 and leaves[8] == np.float32(2.0 ** 0.6)
    new, mp = R.update(leaves, [8, 1, 8], [0.5, 3.0, 0.5], 1e-6, 0.6, 2.0)
    assert mp == 3.0 + 1e-6
    np.testing.assert_allclose(new[[1, 8]], [(3.0 + 1e-6) ** 0.6, (0.5 + 1e-6) ** 0.6],
                               rtol=1e-14)
    assert new[0] == leaves[0] and R.update(leaves, [1], [0.1], 1e-6, 0.6, 2.0)[1] == 2.0


# ---- the package side ---------------------------------------------------------------------
def test_tree_shape_agrees_across_the_abi():
    """per.py's level table, the reference's and the library's node count."""
    from xagents_amd import _lib
    from xagents_amd.per import tree_levels
    lib = _lib.load()
    for L in (1, 64, 65, 70, 4096, 4097, 64 ** 3 + 1, 10 ** 6):
        sizes = R.level_sizes(L)
        levels = tree_levels(L)
        assert [n for n, _ in levels] == sizes
        assert [off for _, off in levels] == list(np.cumsum([0] + sizes[:-1]))
        assert lib.xa_per_tree_nodes(L) == sum(sizes)
    assert lib.xa_per_tree_nodes(0) == 0


def test_abi_symbols_resolve_with_declared_types():
    from xagents_amd import _lib
    header = (ROOT / 'include' / 'xagents_hip.h').read_text()
    lib = _lib.load()
    for name in PER_SYMBOLS:
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
    assert 'batch-max' in header.lower() or 'BATCH-MAX' in header


def test_prioritized_is_refused_where_no_path_takes_it(monkeypatch):
    """DDPG, TD3 and ACER raise in the constructor before they touch their arguments; so do
    DQN and SAC inside an initialised process group."""
    import torch.distributed as dist
    from xagents_amd import ACER, DDPG, DQN, SAC, TD3
    for cls in (DDPG, TD3):
        with pytest.raises(NotImplementedError, match='prioritized'):
            cls(None, None, None, None, prioritized=True)
    with pytest.raises(NotImplementedError, match='prioritized'):
        ACER(None, None, None, prioritized=True)
    monkeypatch.setattr(dist, 'is_available', lambda: True)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    with pytest.raises(NotImplementedError, match='data-parallel'):
        DQN(None, None, None, prioritized=True)
    with pytest.raises(NotImplementedError, match='data-parallel'):
        SAC(None, None, None, None, prioritized=True, data_parallel=False)


def test_sampler_rejects_bad_exponents():
    from xagents_amd.per import PrioritizedSampler
    for kw in (dict(alpha=-0.1), dict(beta=-1.0), dict(eps=0.0)):
        with pytest.raises(ValueError):
            PrioritizedSampler(None, **kw)
