"""Float64 restatement of quantile-regression DQN's head arithmetic (csrc/qr.hip, stated in
csrc/qr_terms.hpp): mean Q and its greedy action, the target quantiles, the pairwise
quantile-Huber terms, the per-sample loss, the gradient of the batch-mean loss, the priority
and the importance weights. numpy only.

Layout: a network output row is [A][N], action-major; tau_hat_i = (2 i + 1) / (2 N).

`case` is the fixed-input generator the GPU tests draw from. For what it returns it
guarantees (and asserts, so a shape it cannot serve raises instead of returning):
* every pair of mean-Q values an argmax compares (theta, theta_next_target,
  theta_next_online; every row) is at least MARGIN = 1e-3 apart;
* row 0 is done (B > 1: the last row is not);
* at least one pair has |u| > kappa and at least one |u| < kappa;
* theta[0][a_0][0] equals y_0 of row 0 exactly (u = 0: L' = 0 there, so the indicator's
  value is immaterial).
With kappa > 0 the gradient is continuous in u, so nothing is excluded from any comparison.

`bounds` derives the f32-versus-f64 tolerances from the arithmetic (eps = 2^-24), with
S = max|theta_next_target| + max|rewards| + max|theta| bounding every |y|, |theta|, |u|:
* mean Q: a lane-strided sum (<= 4 adds), the 6-level wave tree, one divide: 11 roundings of
  values bounded by max|theta|                                         -> 12 eps max|theta|
* u = y - theta with y = v gamma + r: <= 2 eps (|v| + |r|) on y, eps |u| on the
  difference                                                           -> d_u = 3 eps S
* one gradient term w L' / kappa (|.| <= 1): tau_hat and w one rounding each (2 eps), L'
  Lipschitz-1 in u (d_u / kappa), multiply and divide (2 eps); where f32 and f64 disagree on
  [u < 0], |u| <= d_u and both terms are within d_u / kappa of 0      -> 2 d_u / kappa + 4 eps
* its j-sum of N terms (<= N eps relative to their mean after / N), the divides by N and B,
  the weight: 4 more eps
      gradient: (6 eps S / kappa + (N + 8) eps) / B
* one rho = w L / kappa (<= S): L Lipschitz-kappa in u and its own <= 4 roundings, w, multiply,
  divide -> 2 d_u + 8 eps S; the j-sum, / N, the i-sum through lanes and tree (<= 10 adds),
  the weight
      loss: N (N + 26) eps S
* td_abs: two means (11 and 12 eps S with y's own 2 eps S), the difference (2 eps S)
      td_abs: 28 eps S
"""
import numpy as np

MARGIN = 1e-3
EPS32 = 2.0 ** -24

# (B, A, N): a single sample, a batch that does not fill a workgroup's four waves, several
# workgroups; one action; N at and around the wave width and the ragged 4-per-lane cases.
# (B, N) = (1, 1) has one pair and cannot hold both |u| > kappa and |u| < kappa.
SHAPES = ((1, 2, 2), (1, 6, 64), (1, 1, 256), (5, 1, 1), (5, 2, 63), (5, 6, 256), (65, 1, 65),
          (65, 2, 200), (65, 6, 2), (65, 2, 1))
KAPPAS = (1.0, 0.25)
GAMMA = 0.99


def tau_hat(N):
    return (2.0 * np.arange(N) + 1.0) / (2.0 * N)


def _rows(x, A, N):
    x = np.asarray(x, np.float64)
    return x.reshape(x.shape[0], A, N)


def mean_q(theta, A, N):
    """Q [B, A] = (sum_i theta[b][a][i]) / N."""
    return _rows(theta, A, N).sum(2) / N


def greedy(theta, A, N):
    """First index of the maximum of the mean Q."""
    return mean_q(theta, A, N).argmax(1)


def margin(theta, A, N):
    """Smallest gap between two mean-Q values of one row (inf for A = 1)."""
    if A == 1:
        return np.inf
    q = np.sort(mean_q(theta, A, N), axis=1)
    return float(np.diff(q, axis=1).min())


def targets(theta_next_t, theta_next_o, rew, done, gamma, A, N):
    """(a* [B], y [B, N]): a* from the target net's mean Q (the online net's when given),
    y_j = theta_next_t[b][a*][j] gamma + r, r where done. gamma enters as the f32 the kernel
    is handed."""
    nt = _rows(theta_next_t, A, N)
    a_star = greedy(theta_next_t if theta_next_o is None else theta_next_o, A, N)
    v = nt[np.arange(nt.shape[0]), a_star]
    v = np.where(np.asarray(done)[:, None] != 0, 0.0, v)
    y = v * np.float64(np.float32(gamma)) + np.asarray(rew, np.float64)[:, None]
    return a_star, y


def huber(u, kappa):
    """(L, L'): 0.5 u^2 / kappa (|u| - 0.5 kappa), clip(u, +-kappa)."""
    au = np.abs(u)
    return (np.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)),
            np.clip(u, -kappa, kappa))


def pairwise(th_a, y, kappa):
    """(u, rho, g) [B, N, N], index [b][i][j]: u = y_j - theta_i, rho = w L / kappa,
    g = w L' / kappa, w = |tau_hat_i - [u < 0]|."""
    N = th_a.shape[1]
    u = y[:, None, :] - th_a[:, :, None]
    L, Lp = huber(u, kappa)
    w = np.abs(tau_hat(N)[None, :, None] - (u < 0))
    return u, w * L / kappa, w * Lp / kappa


def td(theta, theta_next_t, theta_next_o, act, rew, done, gamma, kappa, A, N, weights=None):
    """Everything xa_qr_td_grad writes, in float64: dict(a_star, y, u, loss [B],
    dtheta [B, A N] (the gradient of the batch mean), td_abs [B])."""
    kappa = np.float64(np.float32(kappa))
    th = _rows(theta, A, N)
    B = th.shape[0]
    rows = np.arange(B)
    act = np.asarray(act, np.int64)
    a_star, y = targets(theta_next_t, theta_next_o, rew, done, gamma, A, N)
    th_a = th[rows, act]
    u, rho, g = pairwise(th_a, y, kappa)
    loss = (rho.sum(2) / N).sum(1)
    d = np.zeros_like(th)
    d[rows, act] = -(g.sum(2) / N) / B
    td_abs = np.abs(y.sum(1) / N - th_a.sum(1) / N)
    if weights is not None:
        w = np.asarray(weights, np.float64)
        loss, d = loss * w, d * w[:, None, None]
    return dict(a_star=a_star, y=y, u=u, loss=loss, dtheta=d.reshape(B, A * N), td_abs=td_abs)


def batch_mean_loss(theta, theta_next_t, theta_next_o, act, rew, done, gamma, kappa, A, N,
                    weights=None):
    """The scalar dtheta is the gradient of."""
    return td(theta, theta_next_t, theta_next_o, act, rew, done, gamma, kappa, A, N,
              weights)['loss'].mean()


def bounds(c, kappa):
    """The derived tolerances (module docstring) of a case: dict(q_mean, grad, loss, td_abs)."""
    B, N = c['B'], c['N']
    tmax = float(np.abs(c['theta']).max())
    S = float(np.abs(c['next_t']).max() + np.abs(c['rew']).max()) + tmax
    qmax = max(tmax, float(np.abs(c['next_t']).max()), float(np.abs(c['next_o']).max()))
    return dict(q_mean=12 * EPS32 * qmax,
                grad=(6 * EPS32 * S / kappa + (N + 8) * EPS32) / B,
                loss=N * (N + 26) * EPS32 * S,
                td_abs=28 * EPS32 * S)


def _net_rows(rng, B, A, N):
    """[B, A N] f64: per action a zero-mean pattern in (-1, 1) on a level; the levels of one
    row are >= 0.007 apart."""
    pat = rng.uniform(-0.5, 0.5, (B, A, N))
    pat -= pat.mean(2, keepdims=True)
    level = np.stack([rng.permutation(A) + rng.uniform(0.0, 0.3, A) for _ in range(B)]) * 0.01
    return pat + level[:, :, None]


def case(B, A, N, kappa, seed=0):
    """The fixed inputs of shape (B, A, N) for threshold kappa (f32 arrays; act int32)."""
    assert B * N >= 2, 'one pair cannot be both above and below kappa'
    rng = np.random.default_rng(100000 * B + 1000 * A + N + seed)
    act = rng.integers(0, A, B).astype(np.int32)
    theta = _net_rows(rng, B, A, N)
    if N >= 2:
        # row 0, taken action: the last quantile >= 2 kappa away from the first, the mean kept
        row = theta[0, act[0]]
        m = row.mean()
        row[N - 1] += 2.0 * kappa + 1.0
        row += m - row.mean()
    theta = theta.reshape(B, A * N).astype(np.float32)
    next_t = _net_rows(rng, B, A, N).reshape(B, A * N).astype(np.float32)
    next_o = _net_rows(rng, B, A, N).reshape(B, A * N).astype(np.float32)
    rew = rng.normal(size=B).astype(np.float32)
    done = (rng.random(B) < 0.3).astype(np.float32)
    done[0] = 1.0
    rew[0] = theta[0, act[0] * N]  # y_j = r exactly where done: u = 0 at quantile 0
    if B > 1:
        done[-1] = 0.0
        rew[-1] = np.float32(4.0 + 2.0 * kappa)  # |y| >= 4 + 2 kappa - 1.06: |u| > kappa
    w = rng.uniform(0.05, 1.0, B).astype(np.float32)
    c = dict(B=B, A=A, N=N, theta=theta, next_t=next_t, next_o=next_o, act=act, rew=rew,
             done=done, weights=w)
    check_case(c, kappa)
    return c


def check_case(c, kappa):
    """The generator's guarantees, asserted on the float64 restatement (and the exact hit in
    f32 as well)."""
    A, N = c['A'], c['N']
    for key in ('theta', 'next_t', 'next_o'):
        assert margin(c[key], A, N) >= MARGIN, key
    assert c['done'][0] == 1.0 and (c['B'] == 1 or c['done'][-1] == 0.0)
    for online in (None, c['next_o']):
        r = td(c['theta'], c['next_t'], online, c['act'], c['rew'], c['done'], GAMMA, kappa,
               A, N)
        au = np.abs(r['u'])
        assert (au > kappa).any() and (au < kappa).any()
        assert r['u'][0, 0, 0] == 0.0
    assert c['rew'][0] == c['theta'][0, c['act'][0] * N]
