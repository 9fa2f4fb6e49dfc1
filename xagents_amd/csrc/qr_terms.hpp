// The per-sample arithmetic of quantile-regression DQN (Dabney et al., arXiv:1710.10044),
// stated once for the kernels of qr.hip: the mean over an action's quantiles and its greedy
// action, the target quantiles, the pairwise quantile-Huber terms (the paper's Eq. 9 and 10,
// normalised by 1 / kappa) and what a sample's loss, gradient row and priority are made of.
// The library is built with -ffp-contract=off, so the f32 operation order written here is the
// contract (tests/qr_ref.py restates it in float64). The Huber branch, the TD target, the
// importance weight and the first-maximum rule are td_terms.hpp's.
//
// Layout: a network output row theta is [A][N], action-major and quantile-minor (output
// a * N + i is quantile i of action a). One wave works on one row: lane l owns the quantiles
// i = l, l + 64, ... of an action, at most kOwned of them.
#pragma once
#include "td_terms.hpp"
#include "xa_common.hpp"

namespace xa_qr {

constexpr int kLanes = 64;
constexpr int kMaxQuantiles = 256;
constexpr int kOwned = kMaxQuantiles / kLanes;  // quantiles a lane owns, at most

// quantile midpoint tau_hat_i = (2 i + 1) / (2 N) (the paper's Lemma 2)
XA_DEV float tau_hat(int i, int N) { return (float)(2 * i + 1) / (float)(2 * N); }

// (sum_i v[i]) / N: lane l adds i = l, l + 64, ... ascending, the lanes by xa_wave_sum's tree,
// one divide. Wave-uniform; every lane of the wave calls it. v: global memory or LDS.
XA_DEV float mean_of(const float* v, int N, int lane) {
  float s = 0.0f;
  for (int i = lane; i < N; i += kLanes) s = s + v[i];
  return xa_wave_sum(s) / (float)N;
}

// first index of the maximum of Q[a] = mean_of(row + a N) (xa_td::argmax_first's rule on the
// means, formed one action at a time: A is not bounded); q_mean [A] (optional) receives them
XA_DEV int greedy(const float* row, int A, int N, int lane, float* q_mean) {
  int best = 0;
  float bv = 0.0f;
  for (int a = 0; a < A; ++a) {
    const float q = mean_of(row + (size_t)a * N, N, lane);
    if (q_mean && lane == 0) q_mean[a] = q;
    if (a == 0 || q > bv) {
      bv = q;
      best = a;
    }
  }
  return best;
}

// target quantile j: the DQN target on quantile j of the next state's greedy action
XA_DEV float target(float theta_next, float done, float gamma, float r) {
  return xa_td::dqn_target(theta_next, done, gamma, r);
}

// One (i, j) pair, u = y_j - theta_i: rho = w L / kappa and the gradient's term w L' / kappa
// with L, L' xa_td::td_term's Huber branch (kappa > 0) and w = |tau_hat_i - [u < 0]|
XA_DEV void pair_terms(float y, float theta, float tau, float kappa, float& rho, float& g) {
  const float u = y - theta;
  float lp;
  const float l = xa_td::td_term(u, kappa, lp);
  const float w = fabsf(tau - (u < 0.0f ? 1.0f : 0.0f));
  rho = (w * l) / kappa;
  g = (w * lp) / kappa;
}

// quantile i's share of the sample's loss from its j-ascending sum of rho, and its entry of
// the batch-mean loss's gradient from its j-ascending sum of w L' / kappa
XA_DEV float loss_term(float rho_sum, int N) { return rho_sum / (float)N; }
XA_DEV float grad_of(float g_sum, int N, int B) { return -(g_sum / (float)N) / (float)B; }

// the new priority's |TD error|: of the means, in DQN's units
XA_DEV float td_abs_of(float y_mean, float q_mean) { return xa_td::td_abs_of(y_mean - q_mean); }

}  // namespace xa_qr
