// Categorical DQN's kernels around the layer executor's GEMMs: the greedy action of the
// expected Q, the Bellman projection of the target distribution, and the fused TD head
// (projection, cross-entropy, gradient row, priority). One wave per row, four rows per
// workgroup, no atomics and nothing shared between workgroups, as qr.hip: a batch is tens to
// a few hundred rows of A K <= a few thousand logits, latency-bound like the QR / PER / SAC
// row kernels. The arithmetic is c51_terms.hpp's.
#include "../../include/xagents_hip.h"
#include "c51_terms.hpp"
#include "td_terms.hpp"
#include "xa_common.hpp"

#include <cmath>

namespace {

using xa_c51::kLanes;
using xa_c51::kMaxAtoms;
using xa_c51::kOwned;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kLanes;  // rows per workgroup

// actions[r] = first argmax of the row's expected Q, or the host-drawn action (xa_dqn_act's
// rule)
__global__ __launch_bounds__(kBlock) void c51_act_kernel(const float* __restrict__ logits, int n,
                                                         int A, int K, float v_min, float v_max,
                                                         const int* __restrict__ random_actions,
                                                         int use_random, int* __restrict__ actions,
                                                         float* __restrict__ q_out) {
  const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
  const int r = blockIdx.x * kWaves + wave;  // wave-uniform
  if (r >= n) return;
  if (use_random) {
    if (lane == 0) actions[r] = random_actions[r];
    return;
  }
  const int best =
      xa_c51::greedy(logits + (size_t)r * A * K, A, K, v_min, xa_c51::delta_of(v_min, v_max, K),
                     lane, q_out ? q_out + (size_t)r * A : nullptr);
  if (lane == 0) actions[r] = best;
}

// The projected target distribution of sample b in the wave's owned slots: a* from the
// expected Q of the next state (the online net's logits when given), then xa_c51::project on
// the target net's logits of a* through the wave's two LDS strips.
XA_DEV void target_dist_of(const float* __restrict__ next_t, const float* __restrict__ next_o,
                           const float* __restrict__ rew, const float* __restrict__ done,
                           const float* __restrict__ discounts, int b, int A, int K, float v_min,
                           float v_max, float delta, float gamma, int lane, float* ps, float* bs,
                           float (&m)[kOwned]) {
  const size_t row = (size_t)b * A * K;
  const int a_star = xa_c51::greedy((next_o ? next_o : next_t) + row, A, K, v_min, delta, lane,
                                    nullptr);
  xa_c51::project(next_t + row + (size_t)a_star * K, done[b],
                  xa_td::discount_of(gamma, discounts, b), rew[b], K, v_min, v_max, delta, lane,
                  ps, bs, m);
}

__global__ __launch_bounds__(kBlock) void c51_project_kernel(
    const float* __restrict__ next_t, const float* __restrict__ next_o,
    const float* __restrict__ rew, const float* __restrict__ done,
    const float* __restrict__ discounts, int B, int A, int K, float v_min, float v_max,
    float gamma, float* __restrict__ target_dist) {
  __shared__ float p_strip[kWaves][kMaxAtoms], b_strip[kWaves][kMaxAtoms];
  const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
  const int b = blockIdx.x * kWaves + wave;  // wave-uniform
  if (b >= B) return;
  float m[kOwned];
  target_dist_of(next_t, next_o, rew, done, discounts, b, A, K, v_min, v_max,
                 xa_c51::delta_of(v_min, v_max, K), gamma, lane, p_strip[wave], b_strip[wave], m);
#pragma unroll
  for (int k = 0; k < kOwned; ++k) {
    const int i = lane + k * kLanes;
    if (i < K) target_dist[(size_t)b * K + i] = m[k];
  }
}

// Sample b's wave: the target distribution m (projected here, or read from target_dist), the
// softmax of the taken action's online logits, then the loss, the whole [A K] gradient row
// (zero off the taken action) and the priority.
__global__ __launch_bounds__(kBlock) void c51_td_kernel(
    const float* __restrict__ logits, const float* __restrict__ next_t,
    const float* __restrict__ next_o, const float* __restrict__ target_dist,
    const int* __restrict__ act, const float* __restrict__ rew, const float* __restrict__ done,
    int B, int A, int K, float v_min, float v_max, float gamma, float* __restrict__ dlogits,
    float* __restrict__ loss, int* __restrict__ adam_step, const float* __restrict__ is_weights,
    float* __restrict__ td_abs, const float* __restrict__ discounts) {
  __shared__ float p_strip[kWaves][kMaxAtoms], b_strip[kWaves][kMaxAtoms];
  const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
  if (adam_step && blockIdx.x == 0 && threadIdx.x == 0)
    adam_step[0] += 1;  // the update's t += 1, one launch fewer
  const int b = blockIdx.x * kWaves + wave;  // wave-uniform
  if (b >= B) return;
  const float delta = xa_c51::delta_of(v_min, v_max, K);
  float m[kOwned];
  if (target_dist) {
#pragma unroll
    for (int k = 0; k < kOwned; ++k) {
      const int i = lane + k * kLanes;
      m[k] = i < K ? target_dist[(size_t)b * K + i] : 0.0f;
    }
  } else {
    target_dist_of(next_t, next_o, rew, done, discounts, b, A, K, v_min, v_max, delta, gamma,
                   lane, p_strip[wave], b_strip[wave], m);
  }

  const size_t row = (size_t)b * A * K;
  const int ab = act[b];
  xa_c51::Softmax s;
  xa_c51::softmax(logits + row + (size_t)ab * K, K, lane, s);
  const float log_S = xa_logf(s.S);
  float lt[kOwned], dth[kOwned];
#pragma unroll
  for (int k = 0; k < kOwned; ++k) {
    lt[k] = xa_c51::loss_term(m[k], s.log_p(k, log_S));
    dth[k] = xa_td::weighted(xa_c51::grad_of(s.p(k), m[k], B), is_weights, b);
  }
  const float l = -xa_c51::owned_sum(lt, K, lane);
  for (int a = 0; a < A; ++a) {
    float* out = dlogits + row + (size_t)a * K;
#pragma unroll
    for (int k = 0; k < kOwned; ++k) {
      const int i = lane + k * kLanes;
      if (i < K) out[i] = a == ab ? dth[k] : 0.0f;
    }
  }
  const float m_mean = xa_c51::mean_of(m, K, v_min, delta, lane);
  const float q = xa_c51::expected_q(s, K, v_min, delta, lane);
  if (lane == 0) {
    if (loss) loss[b] = xa_td::weighted(l, is_weights, b);
    if (td_abs) td_abs[b] = xa_c51::td_abs_of(m_mean, q);
  }
}

int row_blocks(int n) { return (n + kWaves - 1) / kWaves; }

bool shape_ok(int n, int A, int K) {
  return n > 0 && A >= 1 && K >= 2 && K <= kMaxAtoms && (int64_t)A * K < (1ll << 31);
}

// a finite support of positive, finite width
bool support_ok(float v_min, float v_max) {
  return std::isfinite(v_min) && std::isfinite(v_max) && v_max > v_min &&
         std::isfinite(v_max - v_min);
}

#define XA_C51_CHECK(name, n_name, n, A, K, v_min, v_max)                                   \
  XA_CHECK_ARG(shape_ok(n, A, K), name ": needs " n_name " > 0, n_actions >= 1 and 2 <= "   \
               "n_atoms <= %d", kMaxAtoms);                                                 \
  XA_CHECK_ARG(support_ok(v_min, v_max), name ": needs finite v_min, v_max with v_max > v_min")

}  // namespace

extern "C" int xa_c51_act(const float* logits, int n, int n_actions, int n_atoms, float v_min,
                          float v_max, const int* random_actions, int use_random, int* actions,
                          float* q_out, void* stream) {
  XA_CHECK_ARG(actions && (use_random ? random_actions != nullptr : logits != nullptr),
               "xa_c51_act: bad arguments");
  XA_C51_CHECK("xa_c51_act", "n", n, n_actions, n_atoms, v_min, v_max);
  hipLaunchKernelGGL(c51_act_kernel, dim3(row_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream,
                     logits, n, n_actions, n_atoms, v_min, v_max, random_actions, use_random,
                     actions, q_out);
  XA_CHECK_LAUNCH("xa_c51_act");
  return 0;
}

extern "C" int xa_c51_project(const float* logits_next_target, const float* logits_next_online,
                              const float* rewards, const float* dones, const float* discounts,
                              int batch, int n_actions, int n_atoms, float v_min, float v_max,
                              float gamma, float* target_dist, void* stream) {
  XA_CHECK_ARG(logits_next_target && rewards && dones && target_dist,
               "xa_c51_project: bad arguments");
  XA_C51_CHECK("xa_c51_project", "batch", batch, n_actions, n_atoms, v_min, v_max);
  hipLaunchKernelGGL(c51_project_kernel, dim3(row_blocks(batch)), dim3(kBlock), 0,
                     (hipStream_t)stream, logits_next_target, logits_next_online, rewards, dones,
                     discounts, batch, n_actions, n_atoms, v_min, v_max, gamma, target_dist);
  XA_CHECK_LAUNCH("xa_c51_project");
  return 0;
}

extern "C" int xa_c51_td_grad(const float* logits, const float* logits_next_target,
                              const float* logits_next_online, const float* target_dist,
                              const int* actions, const float* rewards, const float* dones,
                              int batch, int n_actions, int n_atoms, float v_min, float v_max,
                              float gamma, float* dlogits, float* loss, int* adam_step,
                              const float* is_weights, float* td_abs, const float* discounts,
                              void* stream) {
  XA_CHECK_ARG(logits && actions && dlogits &&
                   (target_dist || (logits_next_target && rewards && dones)),
               "xa_c51_td_grad: bad arguments");
  XA_C51_CHECK("xa_c51_td_grad", "batch", batch, n_actions, n_atoms, v_min, v_max);
  hipLaunchKernelGGL(c51_td_kernel, dim3(row_blocks(batch)), dim3(kBlock), 0,
                     (hipStream_t)stream, logits, logits_next_target, logits_next_online,
                     target_dist, actions, rewards, dones, batch, n_actions, n_atoms, v_min,
                     v_max, gamma, dlogits, loss, adam_step, is_weights, td_abs, discounts);
  XA_CHECK_LAUNCH("xa_c51_td_grad");
  return 0;
}
