// The per-sample arithmetic of the off-policy updates, stated once for the executor kernels
// (offpolicy.hip), the DQN head fused into the row-dot GEMM (gemm.hip dqn_row_step) and the
// persistent TD3 / DDPG launches (td3_update.hip). The library is built with
// -ffp-contract=off, so the f32 operation order written here is the contract: the fused
// launches and the executor kernels agree bit for bit because they call the same lines.
// (The names live in xa_td: xa_polyak and its neighbours are C-ABI entry points.)
#pragma once
#include "../../include/xagents_hip.h"
#include "xa_common.hpp"

namespace xa_td {

// DDPG / TD3 critic target (ddpg/agent.py:104-127, td3/agent.py:66-110):
// y = r + ((1 - d) gamma) tv, tv the target critic's value (TD3: the smaller of the twins)
XA_DEV float critic_target(float r, float done, float gamma, float tv) {
  return r + ((1.0f - done) * gamma) * tv;
}

// loss term l and its derivative d of the TD error e. delta <= 0: MSE (the reference),
// l = e^2, d = 2 e. delta > 0: tf.keras.losses.Huber(delta), l = 0.5 e^2 if |e| <= delta
// else delta (|e| - 0.5 delta), d = clip(e, +-delta). Twin critics sum their terms.
XA_DEV float td_term(float e, float delta, float& d) {
  if (delta > 0.0f) {
    d = fminf(fmaxf(e, -delta), delta);
    const float ae = fabsf(e);
    return ae <= delta ? 0.5f * (e * e) : delta * (ae - 0.5f * delta);
  }
  d = 2.0f * e;
  return e * e;
}

// first index of the row's maximum (tf.argmax; DQN acting and double Q, dqn/agent.py:107-149)
XA_DEV int argmax_first(const float* r, int A) {
  int best = 0;
  float bv = r[0];
  for (int a = 1; a < A; ++a)
    if (r[a] > bv) {
      bv = r[a];
      best = a;
    }
  return best;
}

// DQN target (dqn/agent.py:118-149): y = v' gamma + r, v' = 0 where done
XA_DEV float dqn_target(float v_next, float done, float gamma, float r) {
  if (done != 0.0f) v_next = 0.0f;
  return v_next * gamma + r;
}

// diff = y - Q[a]: the sample's loss l = mean over the A outputs of td_term (y copies Q off
// the action, so one output carries it) and dqa = dl / dQ[a] (MSE: -(2 diff) / A, the bits
// of (-2 diff) / A)
XA_DEV void dqn_td(float diff, float huber, int A, float& dqa, float& l) {
  float d;
  l = td_term(diff, huber, d) / (float)A;
  dqa = -d / (float)A;
}

// Prioritized replay (per.hip): the sample's importance weight scales a gradient seed or a
// loss row in ONE f32 multiply after the unweighted value (no weights: the value itself, the
// unweighted bits), and the new priority's |TD error| is the unclipped one, with Huber too.
XA_DEV float weighted(float x, const float* is_weights, int b) {
  return is_weights ? x * is_weights[b] : x;
}
XA_DEV float td_abs_of(float e) { return fabsf(e); }

// n-step replay (nstep_terms.hpp): the discount dqn_target receives is the sample's own
// gamma^m where the batch carries one, else gamma (no discounts: the one-step bits).
XA_DEV float discount_of(float gamma, const float* discounts, int b) {
  return discounts ? discounts[b] : gamma;
}

// standard normal from Philox4x32-10 (Box-Muller on two 24-bit uniforms, u1 in (0, 1])
XA_DEV float philox_normal(uint32_t i, uint32_t j, uint64_t ctr, uint64_t seed) {
  const xa_u4 r = xa_philox(i, j, (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed,
                            (uint32_t)(seed >> 32));
  const float u1 = ((float)(r.x >> 8) + 1.0f) * 5.9604644775390625e-08f;
  const float u2 = (float)(r.y >> 8) * 5.9604644775390625e-08f;
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// action noise clip(sigma N(0, 1), +-clip) of element (i, j) of draw ctr (TD3 target
// smoothing td3/agent.py:83-91, DDPG exploration ddpg/agent.py:60-71); sigma == 0 draws nothing
XA_DEV float clipped_noise(uint32_t i, uint32_t j, uint64_t ctr, uint64_t seed, float sigma,
                           float clip) {
  if (sigma == 0.0f) return 0.0f;
  const float n = philox_normal(i, j, ctr, seed) * sigma;
  return fminf(fmaxf(n, -clip), clip);
}

// Polyak blend of a target parameter y towards x (ddpg/agent.py:73-85); tau == 1 copies
XA_DEV float polyak(float y, float x, float tau) {
  return tau == 1.0f ? x : (1.0f - tau) * y + tau * x;
}

// layer activation (XA_ACT_*), and dz = d act'(.) from the layer OUTPUT y
XA_DEV float act(float v, int act) {
  if (act == XA_ACT_RELU) return fmaxf(v, 0.0f);
  if (act == XA_ACT_TANH) return xa_tanhf(v);
  return v;
}
XA_DEV float act_grad(float d, float y, int act) {
  if (act == XA_ACT_RELU) return y > 0.0f ? d : 0.0f;
  if (act == XA_ACT_TANH) return d * (1.0f - y * y);
  return d;
}

}  // namespace xa_td
