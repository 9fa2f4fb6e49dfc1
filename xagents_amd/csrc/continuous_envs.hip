// Pendulum-v1 / MountainCarContinuous-v0 step kernel: one env step per launch, one thread
// per env, for the continuous-action agents (DDPG, TD3, Gaussian PPO / A2C on the layer
// executor). Replaces gym's env.step / env.reset inside BaseAgent.step_envs
// (xagents/base.py:388-426, the gym call at base.py:408) for the two ids -- and, given the
// replay step's arguments, the rest of step_envs(store_in_buffers=True) in the same launch:
// what replay_step_small_kernel (offpolicy.hip) does with the one-step record, taken from
// registers instead, so a dynamics env costs one launch per step and not two.
//
// Thread e owns every word of env e (its f64 state, counters, agent state row, ring slot,
// output rows): no workgroup reads a word another one writes, and the reset draw is keyed by
// the env's own episode counter, so there is no shared counter to bump between launches.
#include "../../include/xagents_hip.h"
#include "continuous_envs.hpp"

namespace {

template <int KIND, bool FUSED>
__global__ __launch_bounds__(256) void continuous_step_kernel(XaContinuousStepArgs a,
                                                              XaReplayStepArgs r) {
  using Env = XaContinuousEnv<KIND>;
  constexpr int OBS = Env::kObs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_envs) return;
  double s[2] = {a.state64[(size_t)e * 2], a.state64[(size_t)e * 2 + 1]};
  int el = a.elapsed[e];
  float o[OBS], post[OBS];
  if (!FUSED && a.reset_only) {
    double u[4];
    xa_reset_uniforms(e, a.episode[e], 0ull, a.seed, u);
    Env::reset(s, u);
    el = 0;
    Env::obs(s, post);
#pragma unroll
    for (int k = 0; k < OBS; ++k) a.out_post[(size_t)e * OBS + k] = post[k];
  } else {
    double reward;
    const bool terminated = Env::step(s, (double)a.actions[(size_t)e * a.act_ld], reward);
    el = el + 1;
    const bool done = terminated || el >= a.max_episode_steps;  // gym TimeLimit
    Env::obs(s, o);  // the obs env.step returns (pre-reset)
    if (done) {
      const int ep = a.episode[e] + 1;
      a.episode[e] = ep;
      double u[4];
      xa_reset_uniforms(e, ep, 0ull, a.seed, u);
      Env::reset(s, u);
      el = 0;
    }
    Env::obs(s, post);
    const float rew = (float)reward, d = done ? 1.0f : 0.0f;
    if (!FUSED) {
#pragma unroll
      for (int k = 0; k < OBS; ++k) {
        a.out_obs[(size_t)e * OBS + k] = o[k];
        a.out_post[(size_t)e * OBS + k] = post[k];
      }
      a.out_rew[e] = rew;
      a.out_done[e] = d;
    } else {
      // BaseAgent.step_envs' bookkeeping, as replay_step_small_kernel: the old state is read
      // before the post-step observation replaces it
      float* st = (float*)r.state + (size_t)e * OBS;
      float old[OBS];
#pragma unroll
      for (int k = 0; k < OBS; ++k) old[k] = st[k];
      if (r.ring_states) {
        const int64_t cnt = r.ring_count[e];
        const int64_t slot = (int64_t)e * r.capacity + cnt % r.capacity;
        float* rs = (float*)r.ring_states + slot * OBS;
        float* rn = (float*)r.ring_new_states + slot * OBS;
#pragma unroll
        for (int k = 0; k < OBS; ++k) {
          rs[k] = old[k];
          rn[k] = o[k];
        }
        const uint8_t* src = (const uint8_t*)r.actions + (int64_t)e * r.act_bytes;
        uint8_t* dst = (uint8_t*)r.ring_actions + slot * r.act_bytes;
        for (int64_t b = 0; b < r.act_bytes; ++b) dst[b] = src[b];
        r.ring_rewards[slot] = rew;
        r.ring_dones[slot] = d;
        r.ring_count[e] = r.ring_kind == XA_RING_RB2 ? (cnt < r.capacity ? cnt + 1 : cnt) : cnt + 1;
      }
      if (r.out_states) {
        float* os = (float*)r.out_states + (size_t)e * OBS;
#pragma unroll
        for (int k = 0; k < OBS; ++k) os[k] = old[k];
      }
      if (r.out_new_states) {
        float* on = (float*)r.out_new_states + (size_t)e * OBS;
#pragma unroll
        for (int k = 0; k < OBS; ++k) on[k] = o[k];
      }
#pragma unroll
      for (int k = 0; k < OBS; ++k) st[k] = post[k];
      const int64_t row = (int64_t)e * (r.out_ld > 0 ? r.out_ld : 1);
      if (r.out_rewards) r.out_rewards[row] = rew;
      if (r.out_dones) r.out_dones[row] = d;
      float ep_ret = r.ep_return[e] + rew;
      if (r.done_epret) r.done_epret[row] = d != 0.0f ? ep_ret : 0.0f;
      if (d != 0.0f) ep_ret = 0.0f;
      r.ep_return[e] = ep_ret;
      r.done[e] = d;
    }
  }
  a.state64[(size_t)e * 2] = s[0];
  a.state64[(size_t)e * 2 + 1] = s[1];
  a.elapsed[e] = el;
}

template <int KIND>
void launch(const XaContinuousStepArgs& a, const XaReplayStepArgs* step, hipStream_t stream) {
  const dim3 grid((a.n_envs + 255) / 256), block(256);
  if (step)
    hipLaunchKernelGGL((continuous_step_kernel<KIND, true>), grid, block, 0, stream, a, *step);
  else
    hipLaunchKernelGGL((continuous_step_kernel<KIND, false>), grid, block, 0, stream, a,
                       XaReplayStepArgs{});
}

}  // namespace

extern "C" int xa_continuous_env_step(const XaContinuousStepArgs* env,
                                      const XaReplayStepArgs* step, void* stream) {
  XA_CHECK_ARG(env != nullptr, "xa_continuous_env_step: null env args");
  const XaContinuousStepArgs& a = *env;
  XA_CHECK_ARG(a.env_kind == XA_ENV_PENDULUM || a.env_kind == XA_ENV_MOUNTAINCAR_CONT,
               "xa_continuous_env_step: env_kind %d is neither XA_ENV_PENDULUM nor "
               "XA_ENV_MOUNTAINCAR_CONT", a.env_kind);
  XA_CHECK_ARG(a.n_envs > 0, "xa_continuous_env_step: n_envs must be > 0");
  XA_CHECK_ARG(a.state64 != nullptr, "xa_continuous_env_step: null state64");
  XA_CHECK_ARG(a.elapsed != nullptr, "xa_continuous_env_step: null elapsed");
  XA_CHECK_ARG(a.episode != nullptr, "xa_continuous_env_step: null episode");
  XA_CHECK_ARG(a.max_episode_steps > 0,
               "xa_continuous_env_step: max_episode_steps must be > 0");
  XA_CHECK_ARG(!(a.reset_only && step),
               "xa_continuous_env_step: reset_only cannot be combined with step");
  XA_CHECK_ARG(a.reset_only || a.actions != nullptr,
               "xa_continuous_env_step: a step needs actions");
  XA_CHECK_ARG(a.reset_only || a.act_ld >= 1, "xa_continuous_env_step: act_ld must be >= 1");
  if (!step) {
    XA_CHECK_ARG(a.out_post != nullptr, "xa_continuous_env_step: null out_post (step == NULL)");
    XA_CHECK_ARG(a.reset_only || (a.out_obs && a.out_rew && a.out_done),
                 "xa_continuous_env_step: a step without `step` needs out_obs, out_rew, "
                 "out_done");
  } else {
    const XaReplayStepArgs& r = *step;
    const int obs = a.env_kind == XA_ENV_PENDULUM ? XaContinuousEnv<XA_ENV_PENDULUM>::kObs
                                                  : XaContinuousEnv<XA_ENV_MOUNTAINCAR_CONT>::kObs;
    XA_CHECK_ARG(r.n_envs == a.n_envs, "xa_continuous_env_step: step n_envs %d != env n_envs %d",
                 r.n_envs, a.n_envs);
    XA_CHECK_ARG(r.obs_bytes == 4 * obs,
                 "xa_continuous_env_step: step obs_bytes %lld, this env_kind needs %d",
                 (long long)r.obs_bytes, 4 * obs);
    XA_CHECK_ARG(r.state != nullptr, "xa_continuous_env_step: null step state");
    XA_CHECK_ARG(r.ep_return != nullptr, "xa_continuous_env_step: null step ep_return");
    XA_CHECK_ARG(r.done != nullptr, "xa_continuous_env_step: null step done");
    XA_CHECK_ARG(!r.ring_states || (r.ring_new_states && r.ring_actions && r.ring_rewards &&
                                    r.ring_dones && r.ring_count && r.capacity > 0 &&
                                    r.actions && r.act_bytes > 0),
                 "xa_continuous_env_step: incomplete replay ring");
  }
  if (a.env_kind == XA_ENV_PENDULUM)
    launch<XA_ENV_PENDULUM>(a, step, (hipStream_t)stream);
  else
    launch<XA_ENV_MOUNTAINCAR_CONT>(a, step, (hipStream_t)stream);
  XA_CHECK_LAUNCH("xa_continuous_env_step");
  return 0;
}
