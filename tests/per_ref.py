"""Float64 restatement of prioritized replay's 64-ary sum tree (csrc/per.hip, arithmetic in
csrc/per_terms.hpp): build, mark, stratified sample with given uniforms, importance weights,
update. numpy only.

The tree: level 0 the leaves, level l >= 1 ceil(n_{l-1} / 64) nodes, until a level has one
node (the root). `build` returns the internal levels as a list (level 1 first); `flat` lays
them out as the device's one node array. Sums here run in numpy's order, the device's in the
wave's pairwise order: f64 sums of <= 64 non-negative terms differ by a few ulps.

`sample` returns, beside the leaves it found, each sample's
margin = min over its descent steps of |t - nearest prefix boundary| / root: a sample whose
margin is far above f64 rounding (1e-9 is asserted by the tests that compare slots) cannot
land in another leaf through a different summation order. The boundaries counted are the
prefix sums at which the chosen child changes, S_i of every child with c_i > 0 except the
last such child: at or past the last one's S_i the rule ("none: the last with c_i > 0") takes
the same child, so t = root (1 - 2^-32), which u = 1 - 2^-24 in the last of 256 strata gives,
is as safe as any other, and t = 0 (u = 0 in the first stratum) is exact on both sides."""
import numpy as np

FAN = 64


def level_sizes(n_leaves):
    """Node counts of the internal levels, level 1 first, the root (1) last."""
    out, n = [], int(n_leaves)
    while True:
        n = (n + FAN - 1) // FAN
        out.append(n)
        if n == 1:
            return out


def _parents(level):
    level = np.asarray(level, np.float64)
    n = (len(level) + FAN - 1) // FAN
    padded = np.zeros(n * FAN)
    padded[:len(level)] = level
    return padded.reshape(n, FAN).sum(1)


def build(leaves):
    """The internal levels over `leaves` (level 1 first, [root] last)."""
    levels, cur = [], np.asarray(leaves, np.float64)
    while True:
        cur = _parents(cur)
        levels.append(cur)
        if len(cur) == 1:
            return levels


def flat(levels):
    """The device's node array: every internal level, level 1 first."""
    return np.concatenate(levels)


def mark_slots(count, cap):
    """The slot each env's next append lands in: e * cap + count[e] % cap."""
    count = np.asarray(count, np.int64)
    return np.arange(len(count), dtype=np.int64) * cap + count % cap


def mark(leaves, count, cap, max_priority, alpha):
    """leaves with every env's next slot set to max_priority^alpha (f32, as stored)."""
    out = np.array(leaves, np.float32)
    out[mark_slots(count, cap)] = np.float32(np.float64(max_priority) ** alpha)
    return out


def stored(count, cap):
    """N = sum_e min(count[e], cap)."""
    return int(np.minimum(np.asarray(count, np.int64), cap).sum())


def sample(leaves, u):
    """Stratified descent with the uniforms u [B]: t_j = (j + u_j) / B * root; at a node the
    first child with t < S_i and c_i > 0 (none: the last with c_i > 0), t -= S_{i-1}.
    Returns (slots [B] int64, margin [B])."""
    leaves = np.asarray(leaves, np.float64)
    levels = [leaves] + build(leaves)
    root = levels[-1][0]
    B = len(u)
    slots, margin = np.zeros(B, np.int64), np.zeros(B)
    for j in range(B):
        t = (np.float64(j) + np.float64(u[j])) / np.float64(B) * root
        k, m = 0, np.inf
        for l in range(len(levels) - 1, 0, -1):
            c = levels[l - 1][k * FAN:(k + 1) * FAN]
            S = np.cumsum(c)
            # the boundaries at which the choice changes: S_i of every child that holds
            # something but the last such child (at and beyond its S_i the rule still
            # takes it, and the node's lower edge 0 is the S_{i-1} its parent measured)
            edges = S[np.nonzero(c > 0)[0][:-1]]
            if len(edges):
                m = min(m, np.abs(edges - t).min() / root)
            hit = np.nonzero((t < S) & (c > 0))[0]
            i = int(hit[0]) if len(hit) else int(np.nonzero(c > 0)[0][-1])
            if i > 0:
                t = t - S[i - 1]
            k = k * FAN + i
        slots[j], margin[j] = k, m
    return slots, margin


def sample_brute(leaves, u):
    """The same draw on the flat cumulative sum: the first leaf whose cumulative sum exceeds
    t_j."""
    leaves = np.asarray(leaves, np.float64)
    cs = np.cumsum(leaves)
    B = len(u)
    t = (np.arange(B, dtype=np.float64) + np.asarray(u, np.float64)) / B * cs[-1]
    return np.searchsorted(cs, t, side='right').astype(np.int64)


def weights(leaf_p, root, n_stored, beta):
    """w_j = (N leaf_j / root)^(-beta) over the batch maximum (the batch-max form)."""
    w = (np.float64(n_stored) * np.asarray(leaf_p, np.float64) / np.float64(root)) ** \
        (-np.float64(beta))
    return w / w.max()


def update(leaves, slots, td_abs, eps, alpha, max_priority):
    """(leaves with leaf[slot] = (|td| + eps)^alpha, the running max_priority)."""
    out = np.array(leaves, np.float64)
    p = np.asarray(td_abs, np.float64) + np.float64(eps)
    out[np.asarray(slots, np.int64)] = p ** np.float64(alpha)
    return out, max(float(max_priority), float(p.max()))


# ---- the fixed inputs the GPU tests draw from (tests/test_gpu_per.py) --------------------
SHAPES = ((1, 64), (2, 35), (17, 241))
BATCHES = (1, 7, 256)


def case_leaves(n_envs, cap, seed=0):
    """About half the leaves zero, the rest in (0.01, 2), as f32."""
    rng = np.random.default_rng(1000 * n_envs + cap + seed)
    L = n_envs * cap
    p = rng.uniform(0.01, 2.0, L) * (rng.random(L) < 0.5)
    if not p.any():
        p[L // 2] = 1.0
    return p.astype(np.float32)


U_LO, U_HI = np.float32(0.0), np.float32(1.0 - 2.0 ** -24)  # xa_u01's extremes


def case_uniforms(n_envs, cap, B, flip):
    """Random 24-bit uniforms (what xa_u01 produces) with the extremes in the first and the
    last stratum: (u_0, u_{B-1}) = (0, 1 - 2^-24), or flipped (B = 1: u_0 alone)."""
    rng = np.random.default_rng(77 * n_envs + cap + B)
    u = (rng.integers(0, 1 << 24, B).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    first, last = (U_HI, U_LO) if flip else (U_LO, U_HI)
    u[-1] = last
    u[0] = first
    return u
