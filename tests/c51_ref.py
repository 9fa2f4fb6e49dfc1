"""Float64 restatement of categorical DQN's head arithmetic (csrc/c51.hip, stated in
csrc/c51_terms.hpp): the softmax over atoms, the expected Q and its greedy action, the Bellman
projection of the target distribution in its gather form, the cross-entropy loss, the gradient
of the batch-mean loss, the priority and the importance weights. numpy only.

Layout: a network output row is [A][K] logits, action-major; atom i sits at
z_i = v_min + i delta, delta = (v_max - v_min) / (K - 1).

`case` is the fixed-input generator the GPU tests draw from. For what it returns it
guarantees (and `check_case` asserts, so a shape it cannot serve raises instead of returning):
* every pair of expected-Q values an argmax compares (theta, next_t, next_o; every row) is at
  least MARGIN = 1e-3 apart, and at least four times `bounds`' limit on a Q value apart, so f32
  and f64 take the same argmax;
* row 0 is done (B > 1: the last row is not);
* row 0's reward lies exactly on a support atom: every b_j of that row is an exact integer in
  float64 (the case in which a floor / ceil scatter with l == u loses the mass);
* B >= 3 (one row cannot do both, and row 0 is the done row): row 1's targets clip at v_max
  and row 2's at v_min; on the support (-1, 1) the rewards reach magnitude 3 and whole rows
  clip;
* the per-row discounts `disc` are gamma^m, m cycling through 1, 2, 3, formed in f32 as the
  n-step gather forms them.
The projection, the clip and log-softmax are continuous in every input, so nothing is excluded
from any comparison; only the argmax needs the margins above.
"""
import numpy as np

MARGIN = 1e-3
EPS32 = 2.0 ** -24
GAMMA = 0.99

# (B, A, K): a single sample, a batch that does not fill a workgroup's four waves, several
# workgroups; one action; K at and around the wave width, the ragged 4-per-lane cases and the
# smallest and largest K.
SHAPES = ((1, 2, 2), (1, 6, 64), (1, 1, 256), (5, 2, 51), (5, 2, 63), (5, 6, 256), (65, 1, 65),
          (65, 2, 200), (65, 6, 2))
SUPPORTS = ((-10.0, 10.0), (0.0, 200.0), (-1.0, 1.0))


def support(K, v_min, v_max):
    """(z [K], delta) of the f32 ends the kernel is handed."""
    v_min, v_max = np.float64(np.float32(v_min)), np.float64(np.float32(v_max))
    delta = (v_max - v_min) / (K - 1)
    return v_min + np.arange(K) * delta, delta


def _rows(x, A, K):
    x = np.asarray(x, np.float64)
    return x.reshape(x.shape[0], A, K)


def log_softmax(logits):
    """(log p, p) over the last axis."""
    t = logits - logits.max(-1, keepdims=True)
    S = np.exp(t).sum(-1, keepdims=True)
    return t - np.log(S), np.exp(t) / S


def expected_q(logits, A, K, v_min, v_max):
    """Q [B, A] = sum_i p_i z_i."""
    z, _ = support(K, v_min, v_max)
    return (log_softmax(_rows(logits, A, K))[1] * z).sum(2)


def greedy(logits, A, K, v_min, v_max):
    """First index of the maximum of the expected Q."""
    return expected_q(logits, A, K, v_min, v_max).argmax(1)


def margin(logits, A, K, v_min, v_max):
    """Smallest gap between two expected-Q values of one row (inf for A = 1)."""
    if A == 1:
        return np.inf
    q = np.sort(expected_q(logits, A, K, v_min, v_max), axis=1)
    return float(np.diff(q, axis=1).min())


def grid_positions(rew, done, discounts, K, v_min, v_max):
    """(Tz [B, K] before the clip, b [B, K]): Tz_j = z_j g_b + r_b, z_j counting as 0 where
    done; b_j = (clip(Tz_j) - v_min) / delta."""
    z, delta = support(K, v_min, v_max)
    v = np.where(np.asarray(done)[:, None] != 0, 0.0, z[None, :])
    tz = v * np.asarray(discounts, np.float64)[:, None] + np.asarray(rew, np.float64)[:, None]
    return tz, (np.clip(tz, z[0], np.float64(np.float32(v_max))) - z[0]) / delta


def project(p_next, b):
    """Gather form: m_i = sum_j p'_j max(0, 1 - |b_j - i|)."""
    K = p_next.shape[1]
    hat = np.maximum(0.0, 1.0 - np.abs(b[:, :, None] - np.arange(K)[None, None, :]))
    return (p_next[:, :, None] * hat).sum(1)


def project_scatter(p_next, b):
    """Algorithm 1's floor / ceil scatter, brute force, the mass placed whole when l == u.
    (A clipped b_j can round to K - 1 plus an ulp: its ceiling stays on the grid.)"""
    B, K = p_next.shape
    m = np.zeros((B, K))
    for r in range(B):
        for j in range(K):
            lo, up = int(np.floor(b[r, j])), min(int(np.ceil(b[r, j])), K - 1)
            if lo == up:
                m[r, lo] += p_next[r, j]
            else:
                m[r, lo] += p_next[r, j] * (up - b[r, j])
                m[r, up] += p_next[r, j] * (b[r, j] - lo)
    return m


def _discounts(B, gamma, discounts):
    if discounts is None:
        return np.full(B, np.float64(np.float32(gamma)))
    return np.asarray(discounts, np.float64)


def target_dist(next_t, next_o, rew, done, gamma, A, K, v_min, v_max, discounts=None):
    """Everything xa_c51_project computes: dict(a_star [B], p_next [B, K], tz, b, m [B, K]).
    a* from the target net's expected Q (the online net's when given); gamma enters as the f32
    the kernel is handed, discounts (per row) take its place when given."""
    nt = _rows(next_t, A, K)
    B = nt.shape[0]
    a_star = greedy(next_t if next_o is None else next_o, A, K, v_min, v_max)
    p_next = log_softmax(nt[np.arange(B), a_star])[1]
    tz, b = grid_positions(rew, done, _discounts(B, gamma, discounts), K, v_min, v_max)
    return dict(a_star=a_star, p_next=p_next, tz=tz, b=b, m=project(p_next, b))


def head(theta, m, act, A, K, v_min, v_max, weights=None):
    """The cross-entropy head on a given target distribution m [B, K]: dict(loss [B],
    dtheta [B, A K] (the gradient of the batch mean), td_abs [B], q [B, A])."""
    th = _rows(theta, A, K)
    B = th.shape[0]
    rows = np.arange(B)
    act = np.asarray(act, np.int64)
    z, _ = support(K, v_min, v_max)
    logp, p = log_softmax(th[rows, act])
    loss = -(m * logp).sum(1)
    d = np.zeros_like(th)
    d[rows, act] = (p - m) / B
    td_abs = np.abs((m * z).sum(1) - (p * z).sum(1))
    if weights is not None:
        w = np.asarray(weights, np.float64)
        loss, d = loss * w, d * w[:, None, None]
    return dict(loss=loss, dtheta=d.reshape(B, A * K), td_abs=td_abs,
                q=expected_q(theta, A, K, v_min, v_max))


def td(theta, next_t, next_o, act, rew, done, gamma, A, K, v_min, v_max, weights=None,
       discounts=None):
    """Everything xa_c51_td_grad writes, in float64: target_dist's and head's entries."""
    r = target_dist(next_t, next_o, rew, done, gamma, A, K, v_min, v_max, discounts)
    r.update(head(theta, r['m'], act, A, K, v_min, v_max, weights))
    return r


def bounds(c):
    """The f32-versus-f64 tolerances of a case: dict(q, m, mass, grad, loss, td_abs), absolute,
    per element. First order in eps = 2^-24 (products of two errors are dropped, every count is
    rounded up); xa_expf and xa_logf are within 2.5 ulp = 5 eps relative (tests/test_oracle.py).

    Sizes. K atoms, V = max(|v_min|, |v_max|), W = v_max - v_min, R = max|r|, T the largest
    spread max - min of one action's logits, L = T + ln K >= |log p_i|. Sums run over <= 4
    lane adds and the 6-level tree, 10 roundings.

    * z_i = v_min + i delta: delta carries 2 eps (a subtraction, a divide), i delta one more
      (<= 3 eps W), the add eps V                                  d_z = eps (3 W + V)
    * t_i = theta_i - mx (the max is exact): eps T. e_i = exp(t_i): relative eps T from t_i and
      5 eps of xa_expf                                             r_e = (T + 5) eps
    * S = sum e_i, positive terms: r_e and 10 roundings           r_S = r_e + 10 eps
    * p_i = e_i / S                                                r_p = r_e + r_S + eps
                                                                       = (2 T + 21) eps
    * Q = (sum e_i z_i) / S: each product |e_i z_i| (r_e + eps) + e_i d_z, 10 roundings of
      partial sums <= S V, then the divide |Q| (r_S + eps)        q = V (2 T + 32) eps + d_z
    * Tz_j = clip(z_j g + r): d_z, the product eps V, the add eps (V + R); the clip is
      Lipschitz-1 and its ends are exact                          d_T = d_z + eps (2 V + R)
    * b_j = (Tz_j - v_min) / delta <= K - 1: the subtraction eps W on top of d_T, delta's
      2 eps and the divide's eps relative
          d_b = (K - 1) ((d_T + eps W) / W + 3 eps)
      which grows like (K - 1) max(|v_min|, |v_max|, |r|) / (v_max - v_min)
    * hat(b_j, i) = max(0, 1 - |b_j - i|): Lipschitz-1 in b; where it is not 0 in both
      precisions |b_j - i| <= 1 + d_b, so its two roundings are 2 eps   d_h = d_b + 2 eps
    * m_i = sum_j p'_j hat_ij, j ascending: p'_j (r_p + eps) hat + p'_j d_h per term, and K
      sequential adds of non-negative terms with partial sums <= m_i <= 1
          m = d_b + r_p + (K + 3) eps
      Summed over i: a p'_j reaches at most 3 atoms (2, and a third by rounding), sum_i m_i = 1
          M1 = sum_i |m_i - m64_i| <= 3 d_h + r_p + (K + 1) eps
    * log p_i = t_i - log S: eps T, r_S through the log, 5 eps ln K of xa_logf (1 <= S <= K),
      the subtraction eps L                          d_lp = eps (T + (T + 15) + 5 ln K + L)
    * loss = -sum_i m_i log p_i: M1 L + d_lp sum m_i + eps L per product, 10 roundings of
      partial sums <= L, the weight (<= 1) one more                loss = M1 L + d_lp + 12 eps L
    * dtheta_i = (p_i - m_i) / B: r_p + m, the subtraction, the divide and the weight 3 eps
          grad = (r_p + m + 3 eps) / B
    * td_abs = |sum_i m_i z_i - Q|: M1 V + d_z + 11 eps V for the first mean, q for the
      second, the subtraction 2 eps V                   td_abs = M1 V + d_z + 13 eps V + q

    sum_i m_i = 1 only up to rounding, so dtheta differs from the exact gradient of the loss
    as written, (p_i sum_j m_j - m_i) / B, by p_i |sum m - 1| / B <= M1 / B: `mass` = M1 in
    the kernel's f32, and M1 2^-29 (eps64 = 2^-53 in place of eps) in this restatement, which
    is what test_c51_ref.py's finite differences allow for."""
    K, B = c['K'], c['B']
    v_min, v_max = c['v_min'], c['v_max']
    V, W = max(abs(v_min), abs(v_max)), v_max - v_min
    R = float(np.abs(c['rew']).max())
    T = max(float(np.ptp(_rows(c[k], c['A'], K), axis=2).max())
            for k in ('theta', 'next_t', 'next_o'))
    assert T <= 80.0, 'past this spread e_i underflows and the relative bounds do not hold'
    e, lnK = EPS32, np.log(K)
    L = T + lnK
    d_z = e * (3 * W + V)
    r_p = (2 * T + 21) * e
    q = V * (2 * T + 32) * e + d_z
    d_T = d_z + e * (2 * V + R)
    d_b = (K - 1) * ((d_T + e * W) / W + 3 * e)
    d_h = d_b + 2 * e
    m = d_b + r_p + (K + 3) * e
    M1 = 3 * d_h + r_p + (K + 1) * e
    d_lp = e * (2 * T + 15 + 5 * lnK + L)
    return dict(q=q, m=m, mass=M1, grad=(r_p + m + 3 * e) / B,
                loss=M1 * L + d_lp + 12 * e * L, td_abs=M1 * V + d_z + 13 * e * V + q)


def _net_rows(rng, B, A, K):
    """[B, A K] f64 logits: per action uniform noise in (-0.2, 0.2) on a tilt towards the
    upper atoms of 0.7 per level (the levels of a row are a permutation of 0 .. A - 1, which
    keeps the expected Q values of a row apart) and a per-action offset in (-2, 2), which a
    softmax does not see."""
    x = np.arange(K) / (K - 1) - 0.5
    noise = rng.uniform(-0.2, 0.2, (B, A, K))
    level = np.stack([rng.permutation(A) + rng.uniform(0.0, 0.1, A) for _ in range(B)]) * 0.7
    offset = rng.uniform(-2.0, 2.0, (B, A, 1))
    return noise + level[:, :, None] * x + offset


def step_discounts(B, gamma):
    """[B] f32: gamma^m with m cycling through 1, 2, 3; g = gamma, then g = g gamma in f32."""
    g0 = np.float32(gamma)
    out = np.empty(B, np.float32)
    for b in range(B):
        g = g0
        for _ in range(b % 3):
            g = np.float32(g * g0)
        out[b] = g
    return out


def _atom_reward(K, v_min, v_max):
    """An f32 reward r on the support whose grid position (r - v_min) / delta is an exact
    integer in float64: the middle atom if it serves, else the top one, else v_min itself."""
    z, delta = support(K, v_min, v_max)
    for i in ((K - 1) // 2, K - 1, 0):
        r = np.float32(z[i])
        b = (np.float64(r) - z[0]) / delta
        if b == np.floor(b):
            return r
    raise AssertionError('v_min itself is always on the grid')


def case(B, A, K, v_min, v_max, seed=0):
    """The fixed inputs of shape (B, A, K) on the support [v_min, v_max] (f32 arrays; act
    int32)."""
    assert K >= 2 and np.float32(v_max) > np.float32(v_min)
    W = float(v_max) - float(v_min)
    rng = np.random.default_rng(100000 * B + 1000 * A + K + seed + int(W))
    act = rng.integers(0, A, B).astype(np.int32)
    theta, next_t, next_o = (_net_rows(rng, B, A, K).reshape(B, A * K).astype(np.float32)
                             for _ in range(3))
    # rewards up to 0.3 W in magnitude, on (-1, 1) up to 3: targets leave the support
    rew = (rng.uniform(-1.0, 1.0, B) * (3.0 if W <= 2.0 else 0.3 * W)).astype(np.float32)
    done = (rng.random(B) < 0.3).astype(np.float32)
    done[0] = 1.0
    rew[0] = _atom_reward(K, v_min, v_max)
    if B > 1:
        done[-1] = 0.0
    if B >= 3:
        far = np.float32(3.0 if W <= 2.0 else 0.75 * W)
        done[1] = done[2] = 0.0
        rew[1], rew[2] = far, -far
    w = rng.uniform(0.05, 1.0, B).astype(np.float32)
    c = dict(B=B, A=A, K=K, v_min=float(v_min), v_max=float(v_max), theta=theta, next_t=next_t,
             next_o=next_o, act=act, rew=rew, done=done, weights=w,
             disc=step_discounts(B, GAMMA))
    check_case(c)
    return c


def check_case(c):
    """The generator's guarantees, asserted on the float64 restatement."""
    B, A, K, v_min, v_max = (c[k] for k in ('B', 'A', 'K', 'v_min', 'v_max'))
    limit = bounds(c)['q']
    for key in ('theta', 'next_t', 'next_o'):
        gap = margin(c[key], A, K, v_min, v_max)
        assert gap >= MARGIN and gap >= 4 * limit, (key, gap, limit)
    assert c['done'][0] == 1.0 and (B == 1 or c['done'][-1] == 0.0)
    for disc in (None, c['disc']):
        tz, b = grid_positions(c['rew'], c['done'], _discounts(B, GAMMA, disc), K, v_min, v_max)
        assert (b[0] == np.floor(b[0])).all() and (tz[0] == np.float64(c['rew'][0])).all()
        if B >= 3:
            assert (tz[1] > v_max).any() and (tz[2] < v_min).any()
            assert c['done'][1] == 0.0 and c['done'][2] == 0.0
    want = np.float32(GAMMA) ** (1 + np.arange(B) % 3).astype(np.float64)
    assert c['disc'].dtype == np.float32 and np.abs(c['disc'] - want).max() <= 3 * EPS32
    assert (c['disc'][::3] == np.float32(GAMMA)).all()
