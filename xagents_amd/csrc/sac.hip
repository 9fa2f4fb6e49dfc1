// Soft Actor-Critic's kernels around the layer executor's GEMMs: the squashed-Gaussian
// policy head (sample + log-density, reparameterised gradient), the entropy-regularised twin
// critic target and the actor / temperature seeds. Row-parallel and latency-bound (a batch
// is a few hundred rows of <= a few action elements); the arithmetic is sac_terms.hpp's.
// alpha is read on device from log_alpha by every launch, so captured phases see its
// current value.
#include "../../include/xagents_hip.h"
#include "sac_terms.hpp"
#include "td_terms.hpp"
#include "xa_common.hpp"

namespace {

constexpr int kRowBlock = 64;    // rows (or elements) per workgroup of the row-parallel kernels
constexpr int kSeedBlock = 256;  // the one workgroup of actor_seed_kernel

// one thread per row: the row's A elements in index order, so logp is a fixed-order sum
__global__ __launch_bounds__(kRowBlock) void sac_sample_kernel(
    const float* __restrict__ mean, int64_t ld_mean, const float* __restrict__ log_std,
    int64_t ld_log_std, int n, int A, const float* __restrict__ eps_in,
    const uint64_t* __restrict__ ctr, uint64_t seed, int deterministic,
    float* __restrict__ actions, int64_t ld_actions, float* __restrict__ eps_out,
    float* __restrict__ logp) {
  const int i = blockIdx.x * kRowBlock + threadIdx.x;
  if (i >= n) return;
  // (a given eps or the deterministic head draws nothing: the counter is not read either)
  const uint64_t c = (!eps_in && !deterministic && ctr) ? *ctr : 0ull;
  float lp = 0.0f;
  for (int j = 0; j < A; ++j) {
    const float ls = xa_sac::clamp_log_std(log_std[i * ld_log_std + j]);
    float eps = 0.0f;
    if (!deterministic)
      eps = eps_in ? eps_in[(int64_t)i * A + j]
                   : xa_td::philox_normal((uint32_t)i, (uint32_t)j, c, seed);
    const float u = xa_sac::pre_tanh(mean[i * ld_mean + j], ls, eps);
    actions[i * ld_actions + j] = xa_tanhf(u);
    if (eps_out) eps_out[(int64_t)i * A + j] = eps;
    lp = lp + xa_sac::logp_term(eps, ls, u);
  }
  if (logp) logp[i] = lp;
}

// twin critics against the soft target: xa_critic_td_grad's kernel with
// min(tv1, tv2) - alpha logp' in the target critic's place. is_weights / td_abs (prioritized
// replay, both optional): td_terms.hpp's weighted / td_abs_of, the twins' mean
__global__ __launch_bounds__(kRowBlock) void sac_td_kernel(
    const float* __restrict__ v1, const float* __restrict__ v2, const float* __restrict__ tv1,
    const float* __restrict__ tv2, const float* __restrict__ logp_next,
    const float* __restrict__ log_alpha, const float* __restrict__ rew,
    const float* __restrict__ done, int B, float gamma, float huber, float* __restrict__ dv1,
    float* __restrict__ dv2, float* __restrict__ loss, const float* __restrict__ is_weights,
    float* __restrict__ td_abs) {
  const int b = blockIdx.x * kRowBlock + threadIdx.x;
  if (b >= B) return;
  const float y = xa_sac::critic_target(rew[b], done[b], gamma, tv1[b], tv2[b],
                                        xa_sac::alpha_of(log_alpha), logp_next[b]);
  const float e1 = v1[b] - y, e2 = v2[b] - y;
  float d1, d2;
  float l = xa_td::td_term(e1, huber, d1);
  l = l + xa_td::td_term(e2, huber, d2);
  dv1[b] = xa_td::weighted(d1, is_weights, b);
  dv2[b] = xa_td::weighted(d2, is_weights, b);
  if (loss) loss[b] = xa_td::weighted(l, is_weights, b);
  if (td_abs) td_abs[b] = 0.5f * (xa_td::td_abs_of(e1) + xa_td::td_abs_of(e2));
}

// ONE workgroup whatever B is, so the temperature gradient's sum has one order: thread t
// adds rows t, t + 256, ... in f64, the wave's lanes by xa_wave_sum_f64's tree, the four
// waves as (w0 + w1) + (w2 + w3)
__global__ __launch_bounds__(kSeedBlock) void sac_actor_seed_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ logp,
    const float* __restrict__ log_alpha, int B, float target_entropy, float* __restrict__ dq1,
    float* __restrict__ dq2, float* __restrict__ loss, float* __restrict__ dlog_alpha) {
  __shared__ double wave_part[kSeedBlock / 64];
  const float alpha = xa_sac::alpha_of(log_alpha);
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += kSeedBlock) {
    float d1, d2;
    const float l = xa_sac::actor_loss(q1[b], q2[b], alpha, logp[b], B, d1, d2);
    dq1[b] = d1;
    dq2[b] = d2;
    if (loss) loss[b] = l;
    acc = acc + (double)xa_sac::temperature_term(logp[b], target_entropy);
  }
  const double w = xa_wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0 && dlog_alpha)
    dlog_alpha[0] =
        (float)(-((wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3])) / (double)B);
}

// one thread per (row, element)
__global__ __launch_bounds__(kRowBlock) void sac_head_grad_kernel(
    const float* __restrict__ da, int64_t ld_da, const float* __restrict__ actions,
    int64_t ld_actions, const float* __restrict__ eps, const float* __restrict__ log_std,
    int64_t ld_log_std, const float* __restrict__ log_alpha, int B, int A,
    float* __restrict__ dmean, float* __restrict__ dlog_std) {
  const int e = blockIdx.x * kRowBlock + threadIdx.x;
  if (e >= B * A) return;
  const int64_t b = e / A, j = e % A;
  float dm, dl;
  xa_sac::head_grad(da[b * ld_da + j], actions[b * ld_actions + j], eps[e],
                    log_std[b * ld_log_std + j], xa_sac::alpha_of(log_alpha), B, dm, dl);
  dmean[e] = dm;
  dlog_std[e] = dl;
}

int row_blocks(int64_t n) { return (int)((n + kRowBlock - 1) / kRowBlock); }

}  // namespace

extern "C" int xa_sac_sample(const float* mean, int64_t ld_mean, const float* log_std,
                             int64_t ld_log_std, int n, int act_dim, const float* eps_in,
                             const uint64_t* rng_counter, uint64_t seed, int deterministic,
                             float* actions, int64_t ld_actions, float* eps_out, float* logp,
                             void* stream) {
  XA_CHECK_ARG(mean && log_std && actions && n > 0 && act_dim > 0 && ld_mean >= act_dim &&
                   ld_log_std >= act_dim && ld_actions >= act_dim,
               "xa_sac_sample: bad arguments");
  XA_CHECK_ARG(deterministic || eps_in || rng_counter,
               "xa_sac_sample: a draw needs rng_counter (or eps_in / deterministic)");
  hipLaunchKernelGGL(sac_sample_kernel, dim3(row_blocks(n)), dim3(kRowBlock), 0,
                     (hipStream_t)stream, mean, ld_mean, log_std, ld_log_std, n, act_dim, eps_in,
                     rng_counter, seed, deterministic, actions, ld_actions, eps_out, logp);
  XA_CHECK_LAUNCH("xa_sac_sample");
  return 0;
}

extern "C" int xa_sac_td_grad_w(const float* v1, const float* v2, const float* tv1,
                                const float* tv2, const float* logp_next, const float* log_alpha,
                                const float* rewards, const float* dones, int batch, float gamma,
                                float huber_delta, float* dv1, float* dv2, float* loss,
                                const float* is_weights, float* td_abs, void* stream) {
  XA_CHECK_ARG(v1 && v2 && tv1 && tv2 && logp_next && log_alpha && rewards && dones && dv1 &&
                   dv2 && batch > 0,
               "xa_sac_td_grad: bad arguments");
  hipLaunchKernelGGL(sac_td_kernel, dim3(row_blocks(batch)), dim3(kRowBlock), 0,
                     (hipStream_t)stream, v1, v2, tv1, tv2, logp_next, log_alpha, rewards, dones,
                     batch, gamma, huber_delta, dv1, dv2, loss, is_weights, td_abs);
  XA_CHECK_LAUNCH("xa_sac_td_grad");
  return 0;
}

extern "C" int xa_sac_td_grad(const float* v1, const float* v2, const float* tv1,
                              const float* tv2, const float* logp_next, const float* log_alpha,
                              const float* rewards, const float* dones, int batch, float gamma,
                              float huber_delta, float* dv1, float* dv2, float* loss,
                              void* stream) {
  return xa_sac_td_grad_w(v1, v2, tv1, tv2, logp_next, log_alpha, rewards, dones, batch, gamma,
                          huber_delta, dv1, dv2, loss, nullptr, nullptr, stream);
}

extern "C" int xa_sac_actor_seed(const float* q1, const float* q2, const float* logp,
                                 const float* log_alpha, int batch, float target_entropy,
                                 float* dq1, float* dq2, float* loss, float* dlog_alpha,
                                 void* stream) {
  XA_CHECK_ARG(q1 && q2 && logp && log_alpha && dq1 && dq2 && batch > 0,
               "xa_sac_actor_seed: bad arguments");
  hipLaunchKernelGGL(sac_actor_seed_kernel, dim3(1), dim3(kSeedBlock), 0, (hipStream_t)stream, q1,
                     q2, logp, log_alpha, batch, target_entropy, dq1, dq2, loss, dlog_alpha);
  XA_CHECK_LAUNCH("xa_sac_actor_seed");
  return 0;
}

extern "C" int xa_sac_head_grad(const float* da, int64_t ld_da, const float* actions,
                                int64_t ld_actions, const float* eps, const float* log_std,
                                int64_t ld_log_std, const float* log_alpha, int batch,
                                int act_dim, float* dmean, float* dlog_std, void* stream) {
  XA_CHECK_ARG(da && actions && eps && log_std && log_alpha && dmean && dlog_std && batch > 0 &&
                   act_dim > 0 && ld_da >= act_dim && ld_actions >= act_dim &&
                   ld_log_std >= act_dim,
               "xa_sac_head_grad: bad arguments");
  XA_CHECK_ARG((int64_t)batch * act_dim < (1ll << 31),
               "xa_sac_head_grad: batch * act_dim >= 2^31");
  hipLaunchKernelGGL(sac_head_grad_kernel, dim3(row_blocks((int64_t)batch * act_dim)),
                     dim3(kRowBlock), 0, (hipStream_t)stream, da, ld_da, actions, ld_actions, eps,
                     log_std, ld_log_std, log_alpha, batch, act_dim, dmean, dlog_std);
  XA_CHECK_LAUNCH("xa_sac_head_grad");
  return 0;
}
