// The per-sample arithmetic of categorical DQN (C51; Bellemare et al., arXiv:1707.06887),
// stated once for the kernels of c51.hip: the softmax over an action's atoms, the expected Q
// and its greedy action, the Bellman projection of the target distribution onto the fixed
// support (Algorithm 1, as a gather) and what a sample's cross-entropy loss, gradient row and
// priority are made of. The library is built with -ffp-contract=off, so the f32 operation
// order written here is the contract (tests/c51_ref.py restates it in float64). The TD target,
// the per-sample discount, the importance weight and the first-maximum rule are td_terms.hpp's.
//
// Layout: a network output row is [A][K] logits, action-major and atom-minor (output
// a * K + i is atom i of action a), atom i at z_i = v_min + i delta,
// delta = (v_max - v_min) / (K - 1), 2 <= K <= 256. One wave works on one row: lane l owns the
// atoms i = l, l + 64, ... of an action, at most kOwned of them (slot k holds i = l + 64 k).
#pragma once
#include "td_terms.hpp"
#include "xa_common.hpp"

namespace xa_c51 {

constexpr int kLanes = 64;
constexpr int kMaxAtoms = 256;
constexpr int kOwned = kMaxAtoms / kLanes;  // atoms a lane owns, at most

XA_DEV float delta_of(float v_min, float v_max, int K) {
  return (v_max - v_min) / (float)(K - 1);
}
XA_DEV float atom(int i, float v_min, float delta) { return v_min + (float)i * delta; }

// wave maximum, xa_wave_sum's DPP tree with fmaxf (a maximum is the same bits in any order).
// The row broadcasts write rows 1, 3 then 2, 3 only; a lane they do not write keeps its own v.
#define XA_C51_DPP_MAX(v, ctrl, rows)                                                       \
  fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), \
                                                      ctrl, rows, 0xF, false)))
XA_DEV float wave_max(float v) {
  v = XA_C51_DPP_MAX(v, 0xB1, 0xF);
  v = XA_C51_DPP_MAX(v, 0x4E, 0xF);
  v = XA_C51_DPP_MAX(v, 0x141, 0xF);
  v = XA_C51_DPP_MAX(v, 0x140, 0xF);
  v = XA_C51_DPP_MAX(v, 0x142, 0xA);
  v = XA_C51_DPP_MAX(v, 0x143, 0xC);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
#undef XA_C51_DPP_MAX

// sum over a lane's owned slots ascending (slots past K hold nothing), the lanes by
// xa_wave_sum's tree. Wave-uniform; every lane of the wave calls it.
XA_DEV float owned_sum(const float (&v)[kOwned], int K, int lane) {
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < kOwned; ++k)
    if (lane + k * kLanes < K) s = s + v[k];
  return xa_wave_sum(s);
}

// Softmax of the K logits at th, in a lane's owned slots: t_i = th_i - mx (mx the wave max),
// e_i = xa_expf(t_i), S their owned_sum; p_i = e_i / S and log p_i = t_i - xa_logf(S).
struct Softmax {
  float t[kOwned], e[kOwned], S;
  XA_DEV float p(int k) const { return e[k] / S; }
  XA_DEV float log_p(int k, float log_S) const { return t[k] - log_S; }
};
XA_DEV void softmax(const float* th, int K, int lane, Softmax& s) {
  float mx = -__builtin_inff();
#pragma unroll
  for (int k = 0; k < kOwned; ++k) {
    const int i = lane + k * kLanes;
    s.t[k] = i < K ? th[i] : -__builtin_inff();
    mx = fmaxf(mx, s.t[k]);
  }
  mx = wave_max(mx);
#pragma unroll
  for (int k = 0; k < kOwned; ++k) {
    const bool mine = lane + k * kLanes < K;
    s.t[k] = mine ? s.t[k] - mx : 0.0f;
    s.e[k] = mine ? xa_expf(s.t[k]) : 0.0f;
  }
  s.S = owned_sum(s.e, K, lane);
}

// sum_i w_i z_i over the owned slots (owned_sum's order): the mean of a distribution w
XA_DEV float mean_of(const float (&w)[kOwned], int K, float v_min, float delta, int lane) {
  float wz[kOwned];
#pragma unroll
  for (int k = 0; k < kOwned; ++k) wz[k] = w[k] * atom(lane + k * kLanes, v_min, delta);
  return owned_sum(wz, K, lane);
}

// expected Q of a softmax: (sum_i e_i z_i) / S
XA_DEV float expected_q(const Softmax& s, int K, float v_min, float delta, int lane) {
  return mean_of(s.e, K, v_min, delta, lane) / s.S;
}

// first index of the maximum of Q[a] (xa_td::argmax_first's rule on expected Q values formed
// one action at a time: A is not bounded); q_out [A] (optional) receives them
XA_DEV int greedy(const float* row, int A, int K, float v_min, float delta, int lane,
                  float* q_out) {
  int best = 0;
  float bv = 0.0f;
  for (int a = 0; a < A; ++a) {
    Softmax s;
    softmax(row + (size_t)a * K, K, lane, s);
    const float q = expected_q(s, K, v_min, delta, lane);
    if (q_out && lane == 0) q_out[a] = q;
    if (a == 0 || q > bv) {
      bv = q;
      best = a;
    }
  }
  return best;
}

// atom j of the next state moved by the Bellman operator and clipped to the support, as a
// position on the atom grid: b_j = (clip(z_j g + r, v_min, v_max) - v_min) / delta (z_j
// counts as 0 where done, so every atom lands on r)
XA_DEV float grid_pos(int j, float done, float g, float r, float v_min, float v_max,
                      float delta) {
  const float tz =
      fminf(fmaxf(xa_td::dqn_target(atom(j, v_min, delta), done, g, r), v_min), v_max);
  return (tz - v_min) / delta;
}

// the share of the mass at grid position b that atom i receives: the hat max(0, 1 - |b - i|),
// exactly 1 where b is the integer i (Algorithm 1's floor / ceil scatter drops that mass when
// l == u); m_i = sum_j p'_j hat(b_j, i), j ascending
XA_DEV float hat(float b, int i) { return fmaxf(0.0f, 1.0f - fabsf(b - (float)i)); }

// Projection for one wave: the softmax p' of the target logits tq (the greedy next action's)
// and the grid positions go to the wave's LDS strips ps / bs [K], then every lane walks
// j = 0 .. K - 1 (p'_j, b_j LDS broadcast reads) for the atoms it owns.
XA_DEV void project(const float* tq, float done, float g, float r, int K, float v_min,
                    float v_max, float delta, int lane, float* ps, float* bs,
                    float (&m)[kOwned]) {
  Softmax s;
  softmax(tq, K, lane, s);
#pragma unroll
  for (int k = 0; k < kOwned; ++k) {
    const int j = lane + k * kLanes;
    if (j < K) {
      ps[j] = s.p(k);
      bs[j] = grid_pos(j, done, g, r, v_min, v_max, delta);
    }
    m[k] = 0.0f;
  }
  xa_wave_sync();
  const int owned = (K + kLanes - 1) / kLanes;  // wave-uniform, <= kOwned
  for (int j = 0; j < K; ++j) {
    const float p = ps[j], b = bs[j];
#pragma unroll
    for (int k = 0; k < kOwned; ++k)
      if (k < owned) m[k] = m[k] + p * hat(b, lane + k * kLanes);
  }
}

// atom i's share of the sample's cross-entropy (loss[b] = -(their owned_sum)) and its entry
// of the batch-mean loss's gradient
XA_DEV float loss_term(float m, float log_p) { return m * log_p; }
XA_DEV float grad_of(float p, float m, int B) { return (p - m) / (float)B; }

// the new priority's |TD error|: of the means, in DQN's units
XA_DEV float td_abs_of(float m_mean, float q) { return xa_td::td_abs_of(m_mean - q); }

}  // namespace xa_c51
