// Quantile-regression DQN's two kernels around the layer executor's GEMMs: the greedy action
// of the mean over quantiles, and the quantile-Huber TD head (targets, N x N pairwise terms,
// loss, gradient row, priority). One wave per row, four rows per workgroup, no atomics and
// nothing shared between workgroups: a batch is tens to a few hundred rows of A N <= a few
// thousand outputs, latency-bound like the PER / SAC row kernels. The arithmetic is
// qr_terms.hpp's.
#include "../../include/xagents_hip.h"
#include "qr_terms.hpp"
#include "td_terms.hpp"
#include "xa_common.hpp"

namespace {

using xa_qr::kLanes;
using xa_qr::kMaxQuantiles;
using xa_qr::kOwned;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kLanes;  // rows per workgroup

// actions[r] = first argmax of the row's mean Q, or the host-drawn action (xa_dqn_act's rule)
__global__ __launch_bounds__(kBlock) void qr_act_kernel(const float* __restrict__ theta, int n,
                                                        int A, int N,
                                                        const int* __restrict__ random_actions,
                                                        int use_random, int* __restrict__ actions,
                                                        float* __restrict__ q_mean) {
  const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
  const int r = blockIdx.x * kWaves + wave;  // wave-uniform
  if (r >= n) return;
  if (use_random) {
    if (lane == 0) actions[r] = random_actions[r];
    return;
  }
  const int best = xa_qr::greedy(theta + (size_t)r * A * N, A, N, lane,
                                 q_mean ? q_mean + (size_t)r * A : nullptr);
  if (lane == 0) actions[r] = best;
}

// Sample b's wave: a* from the mean Q of the next state, the N targets into the wave's LDS
// strip, then every lane walks j = 0 .. N - 1 (y_j an LDS broadcast read) for the quantiles
// it owns. The whole [A N] gradient row is written (zero off the taken action).
__global__ __launch_bounds__(kBlock) void qr_td_kernel(
    const float* __restrict__ theta, const float* __restrict__ theta_next_t,
    const float* __restrict__ theta_next_o, const int* __restrict__ act,
    const float* __restrict__ rew, const float* __restrict__ done, int B, int A, int N,
    float gamma, float kappa, float* __restrict__ dtheta, float* __restrict__ loss,
    int* __restrict__ adam_step, const float* __restrict__ is_weights,
    float* __restrict__ td_abs, const float* __restrict__ discounts) {
  __shared__ float y_strip[kWaves][kMaxQuantiles];
  const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
  if (adam_step && blockIdx.x == 0 && threadIdx.x == 0)
    adam_step[0] += 1;  // the update's t += 1, one launch fewer
  const int b = blockIdx.x * kWaves + wave;  // wave-uniform
  if (b >= B) return;
  float* ys = y_strip[wave];
  const size_t row = (size_t)b * A * N;
  const int a_star = xa_qr::greedy((theta_next_o ? theta_next_o : theta_next_t) + row, A, N,
                                   lane, nullptr);
  const float* tq = theta_next_t + row + (size_t)a_star * N;
  const float d = done[b], r = rew[b], g = xa_td::discount_of(gamma, discounts, b);
  for (int j = lane; j < N; j += kLanes) ys[j] = xa_qr::target(tq[j], d, g, r);
  xa_wave_sync();

  const int ab = act[b];
  const float* th = theta + row + (size_t)ab * N;
  const int owned = (N + kLanes - 1) / kLanes;  // wave-uniform, <= kOwned
  float th_i[kOwned], tau[kOwned], rho_sum[kOwned], g_sum[kOwned];
#pragma unroll
  for (int k = 0; k < kOwned; ++k) {
    const int i = lane + k * kLanes;
    th_i[k] = i < N ? th[i] : 0.0f;  // (a quantile past N: computed, never used)
    tau[k] = xa_qr::tau_hat(i, N);
    rho_sum[k] = g_sum[k] = 0.0f;
  }
  for (int j = 0; j < N; ++j) {
    const float y = ys[j];
#pragma unroll
    for (int k = 0; k < kOwned; ++k)
      if (k < owned) {
        float rho, g;
        xa_qr::pair_terms(y, th_i[k], tau[k], kappa, rho, g);
        rho_sum[k] = rho_sum[k] + rho;
        g_sum[k] = g_sum[k] + g;
      }
  }

  float l = 0.0f, dth[kOwned];
#pragma unroll
  for (int k = 0; k < kOwned; ++k) {
    const bool mine = lane + k * kLanes < N;
    if (mine) l = l + xa_qr::loss_term(rho_sum[k], N);
    dth[k] = xa_td::weighted(xa_qr::grad_of(g_sum[k], N, B), is_weights, b);
  }
  l = xa_wave_sum(l);
  for (int a = 0; a < A; ++a) {
    float* out = dtheta + row + (size_t)a * N;
#pragma unroll
    for (int k = 0; k < kOwned; ++k) {
      const int i = lane + k * kLanes;
      if (i < N) out[i] = a == ab ? dth[k] : 0.0f;
    }
  }
  const float y_mean = xa_qr::mean_of(ys, N, lane), q_mean = xa_qr::mean_of(th, N, lane);
  if (lane == 0) {
    if (loss) loss[b] = xa_td::weighted(l, is_weights, b);
    if (td_abs) td_abs[b] = xa_qr::td_abs_of(y_mean, q_mean);
  }
}

int row_blocks(int n) { return (n + kWaves - 1) / kWaves; }

bool shape_ok(int n, int A, int N) {
  return n > 0 && A >= 1 && N >= 1 && N <= kMaxQuantiles &&
         (int64_t)A * N < (1ll << 31);
}

}  // namespace

extern "C" int xa_qr_act(const float* theta, int n, int n_actions, int n_quantiles,
                         const int* random_actions, int use_random, int* actions, float* q_mean,
                         void* stream) {
  XA_CHECK_ARG(actions && (use_random ? random_actions != nullptr : theta != nullptr),
               "xa_qr_act: bad arguments");
  XA_CHECK_ARG(shape_ok(n, n_actions, n_quantiles),
               "xa_qr_act: needs n > 0, n_actions >= 1 and 1 <= n_quantiles <= %d",
               kMaxQuantiles);
  hipLaunchKernelGGL(qr_act_kernel, dim3(row_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream,
                     theta, n, n_actions, n_quantiles, random_actions, use_random, actions,
                     q_mean);
  XA_CHECK_LAUNCH("xa_qr_act");
  return 0;
}

extern "C" int xa_qr_td_grad_n(const float* theta, const float* theta_next_target,
                               const float* theta_next_online, const int* actions,
                               const float* rewards, const float* dones, int batch,
                               int n_actions, int n_quantiles, float gamma, float huber_kappa,
                               float* dtheta, float* loss, int* adam_step,
                               const float* is_weights, float* td_abs, const float* discounts,
                               void* stream) {
  XA_CHECK_ARG(theta && theta_next_target && actions && rewards && dones && dtheta,
               "xa_qr_td_grad: bad arguments");
  XA_CHECK_ARG(shape_ok(batch, n_actions, n_quantiles),
               "xa_qr_td_grad: needs batch > 0, n_actions >= 1 and 1 <= n_quantiles <= %d",
               kMaxQuantiles);
  XA_CHECK_ARG(huber_kappa > 0.0f, "xa_qr_td_grad: huber_kappa must be > 0");
  hipLaunchKernelGGL(qr_td_kernel, dim3(row_blocks(batch)), dim3(kBlock), 0,
                     (hipStream_t)stream, theta, theta_next_target, theta_next_online, actions,
                     rewards, dones, batch, n_actions, n_quantiles, gamma, huber_kappa, dtheta,
                     loss, adam_step, is_weights, td_abs, discounts);
  XA_CHECK_LAUNCH("xa_qr_td_grad");
  return 0;
}

extern "C" int xa_qr_td_grad(const float* theta, const float* theta_next_target,
                             const float* theta_next_online, const int* actions,
                             const float* rewards, const float* dones, int batch, int n_actions,
                             int n_quantiles, float gamma, float huber_kappa, float* dtheta,
                             float* loss, int* adam_step, const float* is_weights,
                             float* td_abs, void* stream) {
  return xa_qr_td_grad_n(theta, theta_next_target, theta_next_online, actions, rewards, dones,
                         batch, n_actions, n_quantiles, gamma, huber_kappa, dtheta, loss,
                         adam_step, is_weights, td_abs, nullptr, stream);
}
