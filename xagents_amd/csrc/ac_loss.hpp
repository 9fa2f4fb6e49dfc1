// The per-sample actor-critic loss terms and their gradient, stated once for every update
// kernel: the tile of xa_ac_grad (ac_tile.hpp), the tile of the persistent PPO update
// (ppo_tile.hpp) and both loops of xa_ac_head_grad (ac_heads.hip). PPO.update_gradients
// (xagents/ppo/agent.py:112-133) and A2C.train_step (xagents/a2c/agent.py:199-214); the tie
// rules are the ones the float64 oracle restates (oracle.ac_loss_grad_f64). Each caller
// keeps its own arithmetic for the advantage, the ratio and the policy head.
#pragma once
#include "xa_common.hpp"

namespace xa_ac {

// pg, vl: the sample's policy and value loss terms (before the mean); dlogp, dv: d loss /
// d log-prob and d loss / d value of loss = sc * (sum over the samples).
// ppo: adv is the normalised advantage, ratio = exp(logp - old logp), c the clip range;
// A2C (!ppo): adv = R - oldv as it is, ratio and c are not read.
// (Results through references, not a struct: the struct's stack slots reorder the
// instructions of the persistent update.)
XA_DEV void ac_loss_terms(bool ppo, float adv, float ratio, float logp, float v, float oldv,
                          float R, float c, float sc, float value_coef, float& pg,
                          float& dlogp, float& vl, float& dv) {
  if (ppo) {
    const float pg1 = -adv * ratio;
    const float pg2 = -adv * fminf(fmaxf(ratio, 1.0f - c), 1.0f + c);
    pg = fmaxf(pg1, pg2);
    // tf.maximum routes the gradient to its first input when x >= y; the second
    // input's gradient passes tf.clip_by_value only inside [lo, hi]
    const bool r_in = ratio >= 1.0f - c && ratio <= 1.0f + c;
    dlogp = (pg1 >= pg2 || r_in) ? (sc * -adv) * ratio : 0.0f;
    const float dvo = v - oldv;
    const float vclip = oldv + fminf(fmaxf(dvo, -c), c);
    const float vl1 = (v - R) * (v - R);
    const float vl2 = (vclip - R) * (vclip - R);
    vl = fmaxf(vl1, vl2);
    // rounding can make oldv + (v - oldv) != v inside the clip range: the clipped
    // branch then still carries the gradient 2 (v_clip - R)
    const float kv = sc * value_coef * 0.5f * 2.0f;
    if (vl1 >= vl2) dv = kv * (v - R);
    else dv = (dvo >= -c && dvo <= c) ? kv * (vclip - R) : 0.0f;
  } else {
    pg = -(adv * logp);
    dlogp = -sc * adv;
    vl = (v - R) * (v - R);
    dv = sc * value_coef * 2.0f * (v - R);
  }
}

}  // namespace xa_ac
