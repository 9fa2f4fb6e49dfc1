// Off-policy hot path pieces around the GEMMs (gemm.hip):
//   * Conv1D input gradient (col2im as a gather, deterministic) with the ReLU gate of
//     the layer below,
//   * DQN epsilon-greedy action selection and TD targets + MSE gradient
//     (xagents/dqn/agent.py:107-171),
//   * replay rings on device: ReplayBuffer1 (deque + random.sample,
//     xagents/utils/buffers.py:59-98) and ReplayBuffer2 (row-0 overwrite when full,
//     buffers.py:101-148) append / gather. The ring position arithmetic that
//     reproduces the reference's index semantics lives on the host; the kernels move
//     the bytes. The n-step gather (nstep_terms.hpp) reads the append counters on the device.
#include "../../include/xagents_hip.h"
#include "env_step.hpp"
#include "nstep_terms.hpp"
#include "td_terms.hpp"
#include "xa_common.hpp"

namespace {

// dAct[row][q][c] = sum_t dcol[(row P + (q - t) / s) (k C) + t C + c] over taps t with
// (q - t) >= 0, (q - t) % s == 0, (q - t) / s < P; then * [gate > 0]
__global__ __launch_bounds__(256) void col2im_kernel(const float* __restrict__ dcol, int rows,
                                                     int P, int k, int s, int C, int W_in,
                                                     const float* __restrict__ gate,
                                                     float* __restrict__ out) {
  const int64_t total = (int64_t)rows * W_in * C;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    // 32-bit index arithmetic (rows * W_in * C < 2^31, checked on the host)
    const unsigned ue = (unsigned)e;
    const unsigned rq = ue / (unsigned)C;
    const int c = (int)(ue - rq * (unsigned)C);
    const unsigned row_u = rq / (unsigned)W_in;
    const int q = (int)(rq - row_u * (unsigned)W_in);
    const int64_t row = row_u;
    float acc = 0.0f;
    for (int t = 0; t < k; ++t) {
      const int d = q - t;
      if (d < 0 || d % s != 0) continue;
      const int p = d / s;
      if (p >= P) continue;
      acc = acc + dcol[((row * P + p) * k + t) * C + c];
    }
    if (gate && !(gate[e] > 0.0f)) acc = 0.0f;
    out[e] = acc;
  }
}

// argmax (first max, tf.argmax) of each row of q [n x A]; rows flagged random take the
// host-drawn action (np.random.randint, dqn/agent.py:114-116)
__global__ void dqn_act_kernel(const float* __restrict__ q, int n, int A,
                               const int* __restrict__ random_actions, int use_random,
                               int* __restrict__ actions) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (use_random) {
    actions[i] = random_actions[i];
    return;
  }
  actions[i] = xa_td::argmax_first(q + (size_t)i * A, A);
}

// DQN.get_targets + the loss gradient (dqn/agent.py:118-171), td_terms.hpp's dqn_target and
// dqn_td on v' = double ? Qt(s')[argmax Q(s')] : max_a Qt(s') (minimize on a [B] loss sums);
// dQ is zero off the action (y copies Q there). is_weights / td_abs (prioritized replay, both
// optional): td_terms.hpp's weighted / td_abs_of; discounts (n-step replay, optional): its
// discount_of
__global__ void dqn_td_kernel(const float* __restrict__ q, const float* __restrict__ q_next_t,
                              const float* __restrict__ q_next_o, const int* __restrict__ act,
                              const float* __restrict__ rew, const float* __restrict__ done,
                              int B, int A, float gamma, float huber, float* __restrict__ dq,
                              float* __restrict__ loss, int* __restrict__ adam_step,
                              const float* __restrict__ is_weights,
                              float* __restrict__ td_abs,
                              const float* __restrict__ discounts) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (adam_step && b == 0) adam_step[0] += 1;  // the update's t += 1, one launch fewer
  if (b >= B) return;
  const float* qt = q_next_t + (size_t)b * A;
  float v;
  if (q_next_o) {
    v = qt[xa_td::argmax_first(q_next_o + (size_t)b * A, A)];
  } else {
    v = qt[0];
    for (int a = 1; a < A; ++a) v = fmaxf(v, qt[a]);
  }
  const float y = xa_td::dqn_target(v, done[b], xa_td::discount_of(gamma, discounts, b), rew[b]);
  const int ab = act[b];
  const float diff = y - q[(size_t)b * A + ab];
  float dqa, l;
  xa_td::dqn_td(diff, huber, A, dqa, l);
  dqa = xa_td::weighted(dqa, is_weights, b);
  for (int a = 0; a < A; ++a) dq[(size_t)b * A + a] = a == ab ? dqa : 0.0f;
  if (loss) loss[b] = xa_td::weighted(l, is_weights, b);
  if (td_abs) td_abs[b] = xa_td::td_abs_of(diff);
}

// this workgroup's share of one item's nb bytes, s -> d, the item spread over blockIdx.x:
// 16-B moves where the size and both addresses allow, bytes otherwise
XA_DEV void ring_copy_item(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t nb) {
  if ((nb & 15) == 0 && ((uintptr_t)s & 15) == 0 && ((uintptr_t)d & 15) == 0) {
    const int64_t n16 = nb >> 4;
    for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < n16; e += (int64_t)gridDim.x * 256)
      reinterpret_cast<uint4*>(d)[e] = reinterpret_cast<const uint4*>(s)[e];
  } else {
    for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < nb; e += (int64_t)gridDim.x * 256)
      d[e] = s[e];
  }
}

// ring[slot[i]] <- src[i] for n_items items of item_bytes each (append)
__global__ __launch_bounds__(256) void ring_scatter_kernel(const uint8_t* __restrict__ src,
                                                           uint8_t* __restrict__ ring,
                                                           const int64_t* __restrict__ slots,
                                                           int n_items, int64_t item_bytes) {
  const int i = blockIdx.y;
  if (i >= n_items) return;
  ring_copy_item(src + (int64_t)i * item_bytes, ring + slots[i] * item_bytes, item_bytes);
}

// dst[i] <- ring[slot[i]] (sample gather, env-major batch order)
__global__ __launch_bounds__(256) void ring_gather_kernel(const uint8_t* __restrict__ ring,
                                                          uint8_t* __restrict__ dst,
                                                          const int64_t* __restrict__ slots,
                                                          int n_items, int64_t item_bytes) {
  const int i = blockIdx.y;
  if (i >= n_items) return;
  ring_copy_item(ring + slots[i] * item_bytes, dst + (int64_t)i * item_bytes, item_bytes);
}

// every field of a sampled batch in one launch: blockIdx.z = field (wave-uniform), the
// field's bytes spread over blockIdx.x as ring_gather_kernel does
__global__ __launch_bounds__(256) void ring_gather_fields_kernel(XaGatherArgs a) {
  const int i = blockIdx.y, f = blockIdx.z;
  if (i >= a.n_items || f >= a.n_fields) return;
  const int64_t nb = a.field[f].item_bytes;
  ring_copy_item(static_cast<const uint8_t*>(a.field[f].ring) + a.slots[i] * nb,
                 static_cast<uint8_t*>(a.field[f].dst) + (int64_t)i * nb, nb);
}

// the n-step transition of every sampled slot in one launch (nstep_terms.hpp states it): the
// grid is the plain gather's, (observation chunks, items). Every wave redoes its item's walk:
// lane k < m_max loads step k's done (and reward), a ballot and find-first give L, and the
// Horner chain runs over readlanes -- at most 64 scalars per wave, L2 hits. The workgroup then
// copies its share of the two observation rows; workgroup x == 0 writes the item's action,
// reward, done and discount. No LDS, no atomics.
__global__ __launch_bounds__(256) void ring_gather_nstep_kernel(XaNstepGatherArgs a) {
  const int item = blockIdx.y;
  if (item >= a.n_items) return;
  const int lane = threadIdx.x & (xa_nstep::kMaxSteps - 1);
  const int64_t cap = a.capacity;
  const int64_t slot = a.slots[item];
  const int64_t env = slot / cap, i = slot - env * cap;
  const int64_t base = env * cap;
  const int m_max = xa_nstep::max_steps(a.ring_count[env], cap, i, a.n_steps);  // wave-uniform
  const bool mine = lane < m_max;
  const int64_t at = base + xa_nstep::wrap(i + (mine ? lane : 0), cap);
  const float d_k = a.ring_dones[at];
  const int L = xa_nstep::last_step(__ballot(mine && d_k != 0.0f), m_max);
  const int64_t last = base + xa_nstep::wrap(i + L, cap);

  const uint8_t* rs = static_cast<const uint8_t*>(a.ring_states);
  const uint8_t* rn = static_cast<const uint8_t*>(a.ring_new_states);
  ring_copy_item(rs + slot * a.obs_bytes, static_cast<uint8_t*>(a.states) + item * a.obs_bytes,
                 a.obs_bytes);
  ring_copy_item(rn + last * a.obs_bytes,
                 static_cast<uint8_t*>(a.new_states) + item * a.obs_bytes, a.obs_bytes);
  if (blockIdx.x != 0) return;
  const uint8_t* ra = static_cast<const uint8_t*>(a.ring_actions) + slot * a.act_bytes;
  uint8_t* da = static_cast<uint8_t*>(a.actions) + item * a.act_bytes;
  for (int64_t e = threadIdx.x; e < a.act_bytes; e += 256) da[e] = ra[e];
  if (threadIdx.x >= xa_nstep::kMaxSteps) return;  // wave 0 owns the scalars
  const int r_k = __float_as_int(a.ring_rewards[at]);
  float R = __int_as_float(__builtin_amdgcn_readlane(r_k, L));
  for (int k = L - 1; k >= 0; --k)
    R = xa_nstep::fold(__int_as_float(__builtin_amdgcn_readlane(r_k, k)), a.gamma, R);
  const float d_L = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d_k), L));
  if (lane == 0) {
    a.rewards[item] = R;
    a.dones[item] = d_L;
    a.discounts[item] = xa_nstep::discount(a.gamma, L + 1);
  }
}

// the Polyak blend of y towards x (td_terms.hpp polyak) over a parameter vector
__global__ __launch_bounds__(256) void polyak_kernel(const float* __restrict__ x,
                                                     float* __restrict__ y, int64_t n,
                                                     float tau) {
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256)
    y[e] = xa_td::polyak(y[e], x[e], tau);
}

__global__ void step_bump_kernel(int* step) { step[0] += 1; }

// dz = dy * act'(y) from the layer output y (td_terms.hpp act_grad); dz may be dy (the
// layer executor's in-place calls), so that pair carries no __restrict__
__global__ __launch_bounds__(256) void act_grad_kernel(const float* __restrict__ y,
                                                       const float* dy, int64_t n, int act,
                                                       float* dz) {
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256)
    dz[e] = xa_td::act_grad(dy[e], y[e], act);
}

// ---- off-policy replay env step + ring store (BaseAgent.step_envs with
// store_in_buffers, xagents/base.py:388-426): the bookkeeping is env_step.hpp's ---------

// elements [lo, hi) (Ts) of env i's observation, spread over the workgroup: the record at
// cursor c supplies the stepped and the post-reset observation
template <typename T>
XA_DEV void replay_move(const XaReplayStepArgs& a, int i, int c, int64_t slot, int64_t lo,
                        int64_t hi) {
  const int64_t rec = (int64_t)i * a.t_rec + c;
  const T* s_new = xa_step_row<const T>(a.rep_obs, rec, a.obs_bytes);
  const T* s_post = xa_step_row<const T>(a.rep_state, rec, a.obs_bytes);
  for (int64_t e = lo + threadIdx.x; e < hi; e += blockDim.x)
    xa_step_move<T>(a, i, slot, e, s_new[e], s_post[e]);
}

// the record's reward and done into env i's scalars, then the cursor moves on
XA_DEV void replay_scalars(const XaReplayStepArgs& a, int i, int c, int64_t slot) {
  const int64_t rec = (int64_t)i * a.t_rec + c;
  xa_step_scalars(a, i, slot, a.rep_rew[rec], a.rep_done[rec]);
  a.cursor[i] = c + 1 < a.t_rec ? c + 1 : 0;
}

// phase 1: frames (grid: byte chunks x envs); every block reads and writes only its own
// byte range of its env, so reading the old state and overwriting it is race-free
__global__ __launch_bounds__(256) void replay_step_frames_kernel(XaReplayStepArgs a,
                                                                 int64_t chunk) {
  const int i = blockIdx.y;
  const int64_t ob = a.obs_bytes;
  const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < ob ? lo + chunk : ob;
  const int c = a.cursor[i];
  const int64_t slot = xa_step_ring_slot(a, i);
  if ((ob & 15) == 0 && (chunk & 15) == 0)
    replay_move<uint4>(a, i, c, slot, lo >> 4, hi >> 4);
  else
    replay_move<uint8_t>(a, i, c, slot, lo, hi);
}

// phase 2: per-env scalars, ring scalars, cursor / counters (one thread per env)
__global__ void replay_step_scalars_kernel(XaReplayStepArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_envs) return;
  replay_scalars(a, i, a.cursor[i], xa_step_ring_slot(a, i));
}

// small observations (vector envs): both phases in ONE launch, one workgroup per env -- the
// frame bytes of env i by its workgroup, then its scalars by thread 0 (the cursor and the
// ring slot are read by every thread before thread 0 advances them behind the barrier)
__global__ __launch_bounds__(256) void replay_step_small_kernel(XaReplayStepArgs a) {
  const int i = blockIdx.x;
  const int64_t ob = a.obs_bytes;
  const int c = a.cursor[i];
  const int64_t slot = xa_step_ring_slot(a, i);
  const uintptr_t bases = (uintptr_t)a.state | (uintptr_t)a.rep_obs | (uintptr_t)a.rep_state |
                          (uintptr_t)a.ring_states | (uintptr_t)a.ring_new_states |
                          (uintptr_t)a.out_states | (uintptr_t)a.out_new_states;
  // 16-B moves (frames: 7056 B = 441 per env) where every address is a 16-B aligned base
  // plus a multiple of ob
  if ((ob & 15) == 0 && (bases & 15) == 0)
    replay_move<uint4>(a, i, c, slot, 0, ob >> 4);
  else
    replay_move<uint8_t>(a, i, c, slot, 0, ob);
  __syncthreads();
  if (threadIdx.x == 0) replay_scalars(a, i, c, slot);
}

// dst[r][c] = src[r][c] for a rows x cols block (concat / column slices of [B, n] rows)
__global__ __launch_bounds__(256) void copy_block_kernel(const float* __restrict__ src,
                                                         int64_t ld_src, float* __restrict__ dst,
                                                         int64_t ld_dst, int rows, int cols) {
  const int64_t total = (int64_t)rows * cols;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / cols, c = e % cols;
    dst[r * ld_dst + c] = src[r * ld_src + c];
  }
}

// out[b][a] = clip(x[b][a] + noise, lo, hi), the noise td_terms.hpp's clipped_noise at
// (b, a): TD3 target smoothing (td3/agent.py:83-91), DDPG exploration (ddpg/agent.py:60-71)
__global__ void noisy_actions_kernel(const float* __restrict__ x, int64_t ld_x, int rows,
                                     int cols, float sigma, float noise_clip, float lo, float hi,
                                     const uint64_t* __restrict__ ctr, uint64_t seed,
                                     float* __restrict__ out, int64_t ld_out,
                                     float* __restrict__ noise_out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * cols) return;
  const int b = e / cols, a = e % cols;
  // (sigma == 0 draws nothing: the counter is not read either)
  const float n = sigma != 0.0f ? xa_td::clipped_noise((uint32_t)b, (uint32_t)a, ctr ? *ctr : 0ull,
                                                       seed, sigma, noise_clip)
                                : 0.0f;
  if (noise_out) noise_out[e] = n;
  out[(int64_t)b * ld_out + a] = fminf(fmaxf(x[(int64_t)b * ld_x + a] + n, lo), hi);
}

// DDPG / TD3 critic targets and loss gradients: td_terms.hpp's critic_target on min(tv1, tv2)
// and its td_term per critic (minimize sums over the batch); loss[b] is the twins' sum
__global__ void critic_td_kernel(const float* __restrict__ v1, const float* __restrict__ v2,
                                 const float* __restrict__ tv1, const float* __restrict__ tv2,
                                 const float* __restrict__ rew, const float* __restrict__ done,
                                 int B, float gamma, float huber, float* __restrict__ dv1,
                                 float* __restrict__ dv2, float* __restrict__ loss) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float tv = tv2 ? fminf(tv1[b], tv2[b]) : tv1[b];
  const float y = xa_td::critic_target(rew[b], done[b], gamma, tv);
  float d1;
  float l = xa_td::td_term(v1[b] - y, huber, d1);
  dv1[b] = d1;
  if (v2) {
    float d2;
    l = l + xa_td::td_term(v2[b] - y, huber, d2);
    dv2[b] = d2;
  }
  if (loss) loss[b] = l;
}

int grid_for(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < 8192 ? (b > 0 ? b : 1) : 8192);
}

// workgroups per item: one 256-thread pass of 16-B chunks each, at most 64
int ring_grid_x(int64_t item_bytes) {
  const int64_t g = ((item_bytes + 15) / 16 + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 64 ? 64 : g));
}

}  // namespace

extern "C" int xa_conv1d_input_grad(const float* dcol, int rows, int positions, int kernel,
                                    int stride, int channels, int width_in, const float* gate,
                                    float* dinput, void* stream) {
  XA_CHECK_ARG(dcol && dinput && rows > 0 && positions > 0 && kernel > 0 && stride > 0 &&
                   channels > 0 && width_in >= (positions - 1) * stride + kernel,
               "xa_conv1d_input_grad: bad arguments");
  const int64_t total = (int64_t)rows * width_in * channels;
  XA_CHECK_ARG(total < (1ll << 31), "xa_conv1d_input_grad: rows * width * channels >= 2^31");
  hipLaunchKernelGGL(col2im_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                     dcol, rows, positions, kernel, stride, channels, width_in, gate, dinput);
  XA_CHECK_LAUNCH("xa_conv1d_input_grad");
  return 0;
}

extern "C" int xa_dqn_act(const float* q, int n, int n_actions, const int* random_actions,
                          int use_random, int* actions, void* stream) {
  XA_CHECK_ARG(actions && n > 0 && n_actions > 0 && (use_random ? random_actions != nullptr : q != nullptr),
               "xa_dqn_act: bad arguments");
  hipLaunchKernelGGL(dqn_act_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, q, n,
                     n_actions, random_actions, use_random, actions);
  XA_CHECK_LAUNCH("xa_dqn_act");
  return 0;
}

extern "C" int xa_dqn_td_grad_n(const float* q, const float* q_next_target,
                                const float* q_next_online, const int* actions,
                                const float* rewards, const float* dones, int batch,
                                int n_actions, float gamma, float huber_delta, float* dq,
                                float* loss, int* adam_step, const float* is_weights,
                                float* td_abs, const float* discounts, void* stream) {
  XA_CHECK_ARG(q && q_next_target && actions && rewards && dones && dq && batch > 0 &&
                   n_actions > 0,
               "xa_dqn_td_grad: bad arguments");
  hipLaunchKernelGGL(dqn_td_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, q,
                     q_next_target, q_next_online, actions, rewards, dones, batch, n_actions,
                     gamma, huber_delta, dq, loss, adam_step, is_weights, td_abs, discounts);
  XA_CHECK_LAUNCH("xa_dqn_td_grad");
  return 0;
}

extern "C" int xa_dqn_td_grad_w(const float* q, const float* q_next_target,
                                const float* q_next_online, const int* actions,
                                const float* rewards, const float* dones, int batch,
                                int n_actions, float gamma, float huber_delta, float* dq,
                                float* loss, int* adam_step, const float* is_weights,
                                float* td_abs, void* stream) {
  return xa_dqn_td_grad_n(q, q_next_target, q_next_online, actions, rewards, dones, batch,
                          n_actions, gamma, huber_delta, dq, loss, adam_step, is_weights, td_abs,
                          nullptr, stream);
}

extern "C" int xa_dqn_td_grad(const float* q, const float* q_next_target,
                              const float* q_next_online, const int* actions,
                              const float* rewards, const float* dones, int batch, int n_actions,
                              float gamma, float huber_delta, float* dq, float* loss,
                              int* adam_step, void* stream) {
  return xa_dqn_td_grad_w(q, q_next_target, q_next_online, actions, rewards, dones, batch,
                          n_actions, gamma, huber_delta, dq, loss, adam_step, nullptr, nullptr,
                          stream);
}

extern "C" int xa_ring_scatter(const void* src, void* ring, const int64_t* slots, int n_items,
                               int64_t item_bytes, void* stream) {
  XA_CHECK_ARG(src && ring && slots && n_items > 0 && item_bytes > 0,
               "xa_ring_scatter: bad arguments");
  const int gx = ring_grid_x(item_bytes);
  hipLaunchKernelGGL(ring_scatter_kernel, dim3(gx, n_items), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)src, (uint8_t*)ring, slots, n_items, item_bytes);
  XA_CHECK_LAUNCH("xa_ring_scatter");
  return 0;
}

extern "C" int xa_ring_gather(const void* ring, void* dst, const int64_t* slots, int n_items,
                              int64_t item_bytes, void* stream) {
  XA_CHECK_ARG(dst && ring && slots && n_items > 0 && item_bytes > 0,
               "xa_ring_gather: bad arguments");
  const int gx = ring_grid_x(item_bytes);
  hipLaunchKernelGGL(ring_gather_kernel, dim3(gx, n_items), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)ring, (uint8_t*)dst, slots, n_items, item_bytes);
  XA_CHECK_LAUNCH("xa_ring_gather");
  return 0;
}

extern "C" int xa_ring_gather_fields(const XaGatherArgs* p, void* stream) {
  XA_CHECK_ARG(p != nullptr, "xa_ring_gather_fields: null args");
  const XaGatherArgs& a = *p;
  XA_CHECK_ARG(a.n_fields > 0 && a.n_fields <= XA_GATHER_MAX_FIELDS && a.n_items > 0 && a.slots,
               "xa_ring_gather_fields: need 1..%d fields, n_items > 0 and slots",
               XA_GATHER_MAX_FIELDS);
  int gx = 1;
  for (int f = 0; f < a.n_fields; ++f) {
    XA_CHECK_ARG(a.field[f].ring && a.field[f].dst && a.field[f].item_bytes > 0,
                 "xa_ring_gather_fields: field %d: null ring / dst or item_bytes <= 0", f);
    const int g = ring_grid_x(a.field[f].item_bytes);
    gx = g > gx ? g : gx;
  }
  hipLaunchKernelGGL(ring_gather_fields_kernel, dim3(gx, a.n_items, a.n_fields), dim3(256), 0,
                     (hipStream_t)stream, a);
  XA_CHECK_LAUNCH("xa_ring_gather_fields");
  return 0;
}

extern "C" int xa_ring_gather_nstep(const XaNstepGatherArgs* p, void* stream) {
  XA_CHECK_ARG(p != nullptr, "xa_ring_gather_nstep: null args");
  const XaNstepGatherArgs& a = *p;
  XA_CHECK_ARG(a.ring_states && a.ring_new_states && a.ring_actions && a.ring_rewards &&
                   a.ring_dones && a.ring_count && a.slots && a.states && a.new_states &&
                   a.actions && a.rewards && a.dones && a.discounts,
               "xa_ring_gather_nstep: null ring, counter, slots or destination");
  XA_CHECK_ARG(a.n_items > 0 && a.obs_bytes > 0 && a.act_bytes > 0 && a.capacity > 0,
               "xa_ring_gather_nstep: n_items, obs_bytes, act_bytes and capacity must be > 0");
  XA_CHECK_ARG(a.ring_kind == XA_RING_DEQUE,
               "xa_ring_gather_nstep: ring kind %d: only the deque ring keeps an env's "
               "consecutive transitions in consecutive slots",
               a.ring_kind);
  XA_CHECK_ARG(a.n_steps >= 1 && a.n_steps <= xa_nstep::kMaxSteps && a.n_steps <= a.capacity,
               "xa_ring_gather_nstep: n_steps %d outside 1 .. min(%d, capacity %lld)", a.n_steps,
               xa_nstep::kMaxSteps, (long long)a.capacity);
  hipLaunchKernelGGL(ring_gather_nstep_kernel, dim3(ring_grid_x(a.obs_bytes), a.n_items),
                     dim3(256), 0, (hipStream_t)stream, a);
  XA_CHECK_LAUNCH("xa_ring_gather_nstep");
  return 0;
}

extern "C" int xa_polyak(const float* src, float* dst, int64_t n, float tau, void* stream) {
  XA_CHECK_ARG(src && dst && n > 0, "xa_polyak: bad arguments");
  hipLaunchKernelGGL(polyak_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, src,
                     dst, n, tau);
  XA_CHECK_LAUNCH("xa_polyak");
  return 0;
}

extern "C" int xa_adam_step_bump(int* adam_step, void* stream) {
  XA_CHECK_ARG(adam_step != nullptr, "xa_adam_step_bump: null step");
  hipLaunchKernelGGL(step_bump_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, adam_step);
  XA_CHECK_LAUNCH("xa_adam_step_bump");
  return 0;
}

extern "C" int xa_activation_grad(const float* y, const float* dy, int64_t n, int act,
                                  float* dz, void* stream) {
  XA_CHECK_ARG(y && dy && dz && n > 0, "xa_activation_grad: bad arguments");
  hipLaunchKernelGGL(act_grad_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, y,
                     dy, n, act, dz);
  XA_CHECK_LAUNCH("xa_activation_grad");
  return 0;
}

extern "C" int xa_replay_env_step(const XaReplayStepArgs* p, void* stream) {
  XA_CHECK_ARG(p != nullptr, "xa_replay_env_step: null args");
  const XaReplayStepArgs& a = *p;
  XA_CHECK_ARG(a.n_envs > 0 && a.t_rec > 0 && a.obs_bytes > 0 && a.rep_obs && a.rep_state &&
                   a.rep_rew && a.rep_done && a.state && a.cursor && a.ep_return && a.done,
               "xa_replay_env_step: bad env arguments");
  XA_CHECK_ARG(!a.ring_states || (a.ring_new_states && a.ring_actions && a.ring_rewards &&
                                  a.ring_dones && a.ring_count && a.capacity > 0 &&
                                  a.actions && a.act_bytes > 0),
               "xa_replay_env_step: incomplete replay ring");
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunk = 4096;
  dim3 grid((unsigned)((a.obs_bytes + chunk - 1) / chunk), a.n_envs);
  // vector observations and single frames up to 32 KB (C3's 84 x 84 frames: 7056 B): one
  // launch, one workgroup per env
  if (a.obs_bytes <= 4096 || (a.obs_bytes <= 32768 && (a.obs_bytes & 15) == 0)) {
    hipLaunchKernelGGL(replay_step_small_kernel, dim3(a.n_envs), dim3(256), 0, s, a);
    XA_CHECK_LAUNCH("xa_replay_env_step (small)");
    return 0;
  }
  hipLaunchKernelGGL(replay_step_frames_kernel, grid, dim3(256), 0, s, a, chunk);
  XA_CHECK_LAUNCH("xa_replay_env_step (frames)");
  hipLaunchKernelGGL(replay_step_scalars_kernel, dim3((a.n_envs + 63) / 64), dim3(64), 0, s, a);
  XA_CHECK_LAUNCH("xa_replay_env_step (scalars)");
  return 0;
}

// tf.keras.losses.MSE(y, pred) over the last axis, gradient of its batch sum
// (optimizer.minimize on a [B] loss, dqn/agent.py:158-171): d = 2 (pred - y) / A
__global__ void mse_grad_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                int B, int A, float* __restrict__ d, float* __restrict__ loss) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float acc = 0.0f;
  for (int a = 0; a < A; ++a) {
    const float e = pred[(size_t)b * A + a] - y[(size_t)b * A + a];
    d[(size_t)b * A + a] = (2.0f * e) / (float)A;
    acc = acc + e * e;
  }
  if (loss) loss[b] = acc / (float)A;
}

extern "C" int xa_mse_grad(const float* pred, const float* target, int batch, int n_out,
                           float* dpred, float* loss, void* stream) {
  XA_CHECK_ARG(pred && target && dpred && batch > 0 && n_out > 0, "xa_mse_grad: bad arguments");
  hipLaunchKernelGGL(mse_grad_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     pred, target, batch, n_out, dpred, loss);
  XA_CHECK_LAUNCH("xa_mse_grad");
  return 0;
}

extern "C" int xa_copy_block(const float* src, int64_t ld_src, float* dst, int64_t ld_dst,
                             int rows, int cols, void* stream) {
  XA_CHECK_ARG(src && dst && rows > 0 && cols > 0 && ld_src >= cols && ld_dst >= cols,
               "xa_copy_block: bad arguments");
  hipLaunchKernelGGL(copy_block_kernel, dim3(grid_for((int64_t)rows * cols)), dim3(256), 0,
                     (hipStream_t)stream, src, ld_src, dst, ld_dst, rows, cols);
  XA_CHECK_LAUNCH("xa_copy_block");
  return 0;
}

extern "C" int xa_noisy_actions(const float* x, int64_t ld_x, int rows, int cols, float sigma,
                                float noise_clip, float lo, float hi, const uint64_t* rng_counter,
                                uint64_t seed, float* out, int64_t ld_out, float* noise_out,
                                void* stream) {
  XA_CHECK_ARG(x && out && rows > 0 && cols > 0, "xa_noisy_actions: bad arguments");
  hipLaunchKernelGGL(noisy_actions_kernel, dim3((rows * cols + 63) / 64), dim3(64), 0,
                     (hipStream_t)stream, x, ld_x, rows, cols, sigma, noise_clip, lo, hi,
                     rng_counter, seed, out, ld_out, noise_out);
  XA_CHECK_LAUNCH("xa_noisy_actions");
  return 0;
}

extern "C" int xa_critic_td_grad(const float* v1, const float* v2, const float* tv1,
                                 const float* tv2, const float* rewards, const float* dones,
                                 int batch, float gamma, float huber_delta, float* dv1,
                                 float* dv2, float* loss, void* stream) {
  XA_CHECK_ARG(v1 && tv1 && rewards && dones && dv1 && batch > 0 && (!v2 || dv2),
               "xa_critic_td_grad: bad arguments");
  hipLaunchKernelGGL(critic_td_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     v1, v2, tv1, tv2, rewards, dones, batch, gamma, huber_delta, dv1, dv2, loss);
  XA_CHECK_LAUNCH("xa_critic_td_grad");
  return 0;
}
