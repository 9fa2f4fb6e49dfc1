"""Prioritized experience replay (Schaul et al., https://arxiv.org/abs/1511.05952) over the
device replay rings: a 64-ary sum tree in HBM addressed by DeviceReplay's global slots
(env * cap + row), sampled and updated on the device (csrc/per.hip, arithmetic in
csrc/per_terms.hpp).

The draw never touches the host: `sample()` leaves the slots, the importance weights and the
leaves it found in fixed device buffers, `DeviceReplay.gather` reads the slots from there, the
weighted TD head (xa_dqn_td_grad_w / xa_sac_td_grad_w) writes |TD error| into `td_abs` and
`update()` turns it into the new priorities. beta and the Philox counter are device scalars,
so a captured learner phase sees the annealed beta and draws fresh numbers on every replay.
The weights are normalised by the BATCH maximum (the largest weight of each batch is 1).
"""
import numpy as np
import torch

from xagents_amd import _lib, kernels
from xagents_amd._lib import call, stream


def tree_levels(n_leaves):
    """[(node count, offset into the node array)] of the internal levels, level 1 first, the
    root last: each level has ceil(previous / 64) nodes (csrc/per_terms.hpp shape_of)."""
    out, n, off = [], int(n_leaves), 0
    while True:
        n = (n + 63) // 64
        out.append((n, off))
        off += n
        if n == 1:
            return out


class PrioritizedSampler:
    """The sum tree of one DeviceReplay and the buffers of one sampled batch.

    leaves [n * cap] f32 (priority^alpha, 0 for a slot never written), nodes f64 (every
    internal level, the root last), max_priority [1] f32 (initially 1), beta [1] f32,
    counter [1] i64 (the Philox draw index), and per batch: slots [B] i64, weights [B] f32,
    leaf_p [B] f32, td_abs [B] f32. Not checkpointed: a restored agent starts with an empty
    tree, as it starts with empty rings."""

    def __init__(self, replay, alpha=0.6, beta=0.4, eps=1e-6, seed=0, batch=None):
        if not alpha >= 0.0:
            raise ValueError(f'alpha must be >= 0, got {alpha}')
        if not beta >= 0.0:
            raise ValueError(f'beta must be >= 0, got {beta}')
        if not eps > 0.0:
            raise ValueError(f'eps must be > 0 (a zero TD error keeps a positive priority), '
                             f'got {eps}')
        self.replay = replay
        self.alpha, self.eps = float(alpha), float(eps)
        self.seed = (int(seed) * 2654435761 + 0x9e37) % 2**64
        self.n_leaves = replay.n * replay.cap
        self.batch = int(batch if batch is not None else replay.n * replay.k)
        dev = replay.device
        n_nodes = _lib.load().xa_per_tree_nodes(self.n_leaves)
        levels = tree_levels(self.n_leaves)
        assert n_nodes == levels[-1][1] + 1, (n_nodes, levels)
        self.levels = levels
        f32 = dict(dtype=torch.float32, device=dev)
        self.leaves = torch.zeros(self.n_leaves, **f32)
        self.nodes = torch.zeros(n_nodes, dtype=torch.float64, device=dev)
        self.max_priority = torch.ones(1, **f32)
        self.beta = torch.full((1,), float(beta), **f32)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.slots = torch.zeros(self.batch, dtype=torch.int64, device=dev)
        self.weights = torch.zeros(self.batch, **f32)
        self.leaf_p = torch.zeros(self.batch, **f32)
        self.td_abs = torch.zeros(self.batch, **f32)

    def set_beta(self, beta):
        """Write the importance exponent into its device scalar (outside any capture)."""
        self.beta.fill_(float(beta))

    def _tree(self):
        return self.leaves.data_ptr(), self.nodes.data_ptr(), self.n_leaves

    def rebuild(self):
        """Every internal node from the leaves (after the leaf array was written whole)."""
        call('xa_per_rebuild', *self._tree(), stream())

    def mark(self):
        """The slot every env's next append lands in gets max_priority^alpha: enqueue right in
        front of the env-step launch that appends (it reads the ring counters before)."""
        r = self.replay
        call('xa_per_mark', *self._tree(), r.count.data_ptr(), r.n, r.cap,
             self.max_priority.data_ptr(), kernels._f32(self.alpha), stream())

    def sample(self, u_in=None, u_out=None):
        """One stratified batch into slots / leaf_p / weights; returns slots. u_in [B] f32
        (device) replaces the Philox uniforms (then the counter does not move), u_out
        receives the uniforms used."""
        r = self.replay
        if not np.any(r.host_count):
            raise ValueError('prioritized sample from empty replay rings: append first')
        call('xa_per_sample', *self._tree(), r.count.data_ptr(), r.n, r.cap, self.batch,
             u_in.data_ptr() if u_in is not None else None, self.counter.data_ptr(), self.seed,
             self.beta.data_ptr(), self.slots.data_ptr(), self.leaf_p.data_ptr(),
             self.weights.data_ptr(), u_out.data_ptr() if u_out is not None else None, stream())
        if u_in is None:
            kernels.counter_bump(self.counter)
        return self.slots

    def update(self):
        """The sampled slots' priorities from td_abs (the weighted TD head's output)."""
        call('xa_per_update', *self._tree(), self.slots.data_ptr(), self.td_abs.data_ptr(),
             self.batch, kernels._f32(self.alpha), kernels._f32(self.eps),
             self.max_priority.data_ptr(), stream())
