// Pendulum-v1 / MountainCarContinuous-v0 step kernel: one env step per launch, one thread
// per env, for the continuous-action agents (DDPG, TD3, Gaussian PPO / A2C on the layer
// executor). Replaces gym's env.step / env.reset inside BaseAgent.step_envs
// (xagents/base.py:388-426, the gym call at base.py:408) for the two ids -- and, given the
// replay step's arguments, the rest of step_envs(store_in_buffers=True) in the same launch:
// the bookkeeping of env_step.hpp that replay_step_small_kernel (offpolicy.hip) does with the
// one-step record, fed from registers instead, so a dynamics env costs one launch per step
// and not two.
//
// Thread e owns every word of env e (its f64 state, counters, agent state row, ring slot,
// output rows): no workgroup reads a word another one writes, and the reset draw is keyed by
// the env's own episode counter, so there is no shared counter to bump between launches.
#include "../../include/xagents_hip.h"
#include "continuous_envs.hpp"
#include "env_step.hpp"

namespace {

// an env's whole observation, one element of xa_step_move. Copied float by float: the
// 12-byte aggregate copy is otherwise a memcpy through a stack slot, which lands in LDS
template <int N>
struct ObsRow {
  float v[N];
  ObsRow() = default;
  XA_DEV ObsRow(const ObsRow& o) { *this = o; }
  XA_DEV ObsRow& operator=(const ObsRow& o) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = o.v[k];
    return *this;
  }
};

template <int KIND, bool FUSED>
__global__ __launch_bounds__(256) void continuous_step_kernel(XaContinuousStepArgs a,
                                                              XaReplayStepArgs r) {
  using Env = XaContinuousEnv<KIND>;
  constexpr int OBS = Env::kObs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_envs) return;
  double s[2] = {a.state64[(size_t)e * 2], a.state64[(size_t)e * 2 + 1]};
  int el = a.elapsed[e];
  ObsRow<OBS> o, post;
  if (!FUSED && a.reset_only) {
    double u[4];
    xa_reset_uniforms(e, a.episode[e], 0ull, a.seed, u);
    Env::reset(s, u);
    el = 0;
    Env::obs(s, post.v);
#pragma unroll
    for (int k = 0; k < OBS; ++k) a.out_post[(size_t)e * OBS + k] = post.v[k];
  } else {
    double reward;
    const bool terminated = Env::step(s, (double)a.actions[(size_t)e * a.act_ld], reward);
    el = el + 1;
    const bool done = terminated || el >= a.max_episode_steps;  // gym TimeLimit
    Env::obs(s, o.v);  // the obs env.step returns (pre-reset)
    if (done) {
      const int ep = a.episode[e] + 1;
      a.episode[e] = ep;
      double u[4];
      xa_reset_uniforms(e, ep, 0ull, a.seed, u);
      Env::reset(s, u);
      el = 0;
    }
    Env::obs(s, post.v);
    const float rew = (float)reward, d = done ? 1.0f : 0.0f;
    if (!FUSED) {
#pragma unroll
      for (int k = 0; k < OBS; ++k) {
        a.out_obs[(size_t)e * OBS + k] = o.v[k];
        a.out_post[(size_t)e * OBS + k] = post.v[k];
      }
      a.out_rew[e] = rew;
      a.out_done[e] = d;
    } else {
      // BaseAgent.step_envs' bookkeeping (env_step.hpp), the env's observation as one element
      const int64_t slot = xa_step_ring_slot(r, e);
      xa_step_move<ObsRow<OBS>>(r, e, slot, 0, o, post);
      xa_step_scalars(r, e, slot, rew, d);
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
