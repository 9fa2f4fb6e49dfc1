// The per-element arithmetic of Soft Actor-Critic (https://arxiv.org/abs/1812.05905), stated
// once for the kernels of sac.hip: the tanh-squashed Gaussian sample and its log-density, the
// entropy-regularised critic target, the actor loss with the critics' seed, the
// reparameterised head gradient and the temperature gradient. The library is built with
// -ffp-contract=off, so the f32 operation order written here is the contract
// (tests/sac_ref.py restates it in float64). The TD error terms are td_terms.hpp's.
#pragma once
#include "td_terms.hpp"
#include "xa_common.hpp"

namespace xa_sac {

constexpr float LOG_STD_MIN = -20.0f;
constexpr float LOG_STD_MAX = 2.0f;
constexpr float LOG_2 = 0.693147180559945309f;
constexpr float HALF_LOG_2PI = 0.918938533204672742f;

// ls = clamp(log_std, LOG_STD_MIN, LOG_STD_MAX); its derivative is 0 strictly outside the
// interval, 1 inside and at the bounds
XA_DEV float clamp_log_std(float log_std) {
  return fminf(fmaxf(log_std, LOG_STD_MIN), LOG_STD_MAX);
}
XA_DEV float clamp_grad(float log_std) {
  return (log_std < LOG_STD_MIN || log_std > LOG_STD_MAX) ? 0.0f : 1.0f;
}

// alpha = exp(log_alpha), read on device by every launch that uses it
XA_DEV float alpha_of(const float* log_alpha) { return xa_expf(log_alpha[0]); }

// softplus(x) = max(x, 0) + log1p(exp(-|x|)): no overflow at either end
XA_DEV float softplus(float x) {
  return fmaxf(x, 0.0f) + xa_logf(1.0f + xa_expf(-fabsf(x)));
}

// pre-squash sample u = mean + exp(ls) eps; the action is xa_tanhf(u)
XA_DEV float pre_tanh(float mean, float ls, float eps) { return mean + xa_expf(ls) * eps; }

// log(1 - tanh(u)^2) = 2 (log 2 - u - softplus(-2 u)), finite for every finite u
XA_DEV float log_one_minus_tanh2(float u) {
  return 2.0f * ((LOG_2 - u) - softplus(-2.0f * u));
}

// element j's share of the row's log-density (no additive epsilon): the row's logp is the
// sum of these in index order
XA_DEV float logp_term(float eps, float ls, float u) {
  return ((-0.5f * (eps * eps) - ls) - HALF_LOG_2PI) - log_one_minus_tanh2(u);
}

// soft value of the next state and the critic target y = r + ((1 - d) gamma) soft
XA_DEV float soft_value(float tv1, float tv2, float alpha, float logp_next) {
  return fminf(tv1, tv2) - alpha * logp_next;
}
XA_DEV float critic_target(float r, float done, float gamma, float tv1, float tv2, float alpha,
                           float logp_next) {
  return xa_td::critic_target(r, done, gamma, soft_value(tv1, tv2, alpha, logp_next));
}

// the row's actor loss alpha logp - min(q1, q2) (the batch loss is the mean over rows) and
// the seeds of the critics' input-gradient passes: d(-mean Qmin)/dq = -1 / B on the critic
// holding the minimum (ties: critic 1), 0 on the other
XA_DEV float actor_loss(float q1, float q2, float alpha, float logp, int B, float& dq1,
                        float& dq2) {
  const float seed = -1.0f / (float)B;
  const bool first = q1 <= q2;
  dq1 = first ? seed : 0.0f;
  dq2 = first ? 0.0f : seed;
  return alpha * logp - fminf(q1, q2);
}

// head gradient of element j: dqa = d(-mean Qmin)/da_j summed over the two critics' input
// gradients, a = tanh(u). du = dqa (1 - a^2) + (alpha / B) 2 a; dmean = du;
// dlog_std = clampgrad (du exp(ls) eps - alpha / B)
XA_DEV void head_grad(float dqa, float a, float eps, float log_std, float alpha, int B,
                      float& dmean, float& dlog_std) {
  const float ab = alpha / (float)B;
  const float du = dqa * (1.0f - a * a) + ab * (2.0f * a);
  dmean = du;
  dlog_std = clamp_grad(log_std) * ((du * xa_expf(clamp_log_std(log_std))) * eps - ab);
}

// temperature: L = -mean(log_alpha (logp + target_entropy)), logp held constant;
// dL/dlog_alpha = -mean(logp + target_entropy). One row's term of that mean:
XA_DEV float temperature_term(float logp, float target_entropy) { return logp + target_entropy; }

}  // namespace xa_sac
