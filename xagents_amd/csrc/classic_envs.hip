// Acrobot-v1 / MountainCar-v0 step kernel: one env step per launch, one thread per env, for
// the agents whose models run on the layer executor (TRPO, and PPO / A2C with non-fused
// models). Replaces gym's env.step / env.reset inside BaseAgent.step_envs
// (xagents/base.py:388-426, the gym call at base.py:408) for the two ids and writes the
// one-step record xa_replay_env_step consumes, as xa_walker_step does. The dynamics are
// csrc/classic_envs.hpp, shared with the fused rollout (mlp_rollout.hip), so the two paths
// agree bit for bit given the same actions, seed, counter and step index.
#include "../../include/xagents_hip.h"
#include "classic_envs.hpp"

namespace {

template <int KIND>
__global__ __launch_bounds__(256) void classic_step_kernel(XaClassicStepArgs a) {
  using Env = XaClassicEnv<KIND>;
  constexpr int OBS = Env::kObs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_envs) return;
  const uint64_t ctr = a.counter ? *a.counter : 0ull;
  double s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = a.state64[(size_t)e * 4 + k];
  int el = a.elapsed[e];
  float o[OBS];
  if (a.reset_only) {
    double u[4];
    xa_reset_uniforms(e, a.t, ctr, a.seed, u);
    Env::reset(s, u);
    el = 0;
  } else {
    const int act = min(max(a.actions[(size_t)e * a.act_ld], 0), Env::kActions - 1);
    const bool terminated = Env::step(s, act);
    el = el + 1;
    const bool done = terminated || el >= a.max_episode_steps;  // gym TimeLimit
    Env::obs(s, o);  // the obs env.step returns (pre-reset)
#pragma unroll
    for (int k = 0; k < OBS; ++k) a.out_obs[(size_t)e * OBS + k] = o[k];
    a.out_rew[e] = Env::reward(terminated);
    a.out_done[e] = done ? 1.0f : 0.0f;
    if (done) {
      double u[4];
      xa_reset_uniforms(e, a.t, ctr, a.seed, u);
      Env::reset(s, u);
      el = 0;
    }
  }
  Env::obs(s, o);
#pragma unroll
  for (int k = 0; k < OBS; ++k) a.out_post[(size_t)e * OBS + k] = o[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) a.state64[(size_t)e * 4 + k] = s[k];
  a.elapsed[e] = el;
}

}  // namespace

extern "C" int xa_classic_step(const XaClassicStepArgs* args, void* stream) {
  XA_CHECK_ARG(args != nullptr, "xa_classic_step: null args");
  const XaClassicStepArgs& a = *args;
  XA_CHECK_ARG(a.env_kind == XA_ENV_ACROBOT || a.env_kind == XA_ENV_MOUNTAINCAR,
               "xa_classic_step: env_kind %d is neither XA_ENV_ACROBOT nor XA_ENV_MOUNTAINCAR",
               a.env_kind);
  XA_CHECK_ARG(a.n_envs > 0, "xa_classic_step: n_envs must be > 0");
  XA_CHECK_ARG(a.state64 != nullptr, "xa_classic_step: null state64");
  XA_CHECK_ARG(a.elapsed != nullptr && a.out_post != nullptr,
               "xa_classic_step: null elapsed / out_post");
  XA_CHECK_ARG(a.max_episode_steps > 0, "xa_classic_step: max_episode_steps must be > 0");
  XA_CHECK_ARG(a.reset_only || (a.actions && a.act_ld >= 1 && a.out_obs && a.out_rew &&
                                a.out_done),
               "xa_classic_step: a step needs actions (act_ld >= 1), out_obs, out_rew, out_done");
  const dim3 grid((a.n_envs + 255) / 256), block(256);
  if (a.env_kind == XA_ENV_ACROBOT)
    hipLaunchKernelGGL(classic_step_kernel<XA_ENV_ACROBOT>, grid, block, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(classic_step_kernel<XA_ENV_MOUNTAINCAR>, grid, block, 0,
                       (hipStream_t)stream, a);
  XA_CHECK_LAUNCH("xa_classic_step");
  return 0;
}
