// BaseAgent.step_envs' bookkeeping (xagents/base.py:388-426 with store_in_buffers) for one
// env of an XaReplayStepArgs, stated once: the replay step kernels (offpolicy.hip) feed it
// from the record, the continuous envs' one-launch step (continuous_envs.hip) from registers.
#pragma once
#include "../../include/xagents_hip.h"
#include "xa_common.hpp"

// The ring row env i's append lands on, -1 without a ring. RB1 deque: after the newest
// element; RB2: row current_size % size, current_size saturating at size -> row 0 once full
// (buffers.py:133-135). Both are count % capacity: xa_step_scalars keeps the count.
XA_DEV int64_t xa_step_ring_slot(const XaReplayStepArgs& a, int i) {
  return a.ring_states ? (int64_t)i * a.capacity + a.ring_count[i] % a.capacity : -1;
}

template <typename T>
XA_DEV T* xa_step_row(const void* base, int64_t row, int64_t row_bytes) {
  return reinterpret_cast<T*>((uint8_t*)base + row * row_bytes);
}

// Element e (a T) of env i's observation: the old state to the ring and out_states, the
// stepped observation nw to ring_new_states and out_new_states, the post-reset observation
// into state. The old element is read before it is overwritten, by the thread that overwrites.
template <typename T>
XA_DEV void xa_step_move(const XaReplayStepArgs& a, int i, int64_t slot, int64_t e, T nw, T post) {
  const int64_t ob = a.obs_bytes;
  T* st = xa_step_row<T>(a.state, i, ob);
  const T old = st[e];
  if (slot >= 0) {
    xa_step_row<T>(a.ring_states, slot, ob)[e] = old;
    xa_step_row<T>(a.ring_new_states, slot, ob)[e] = nw;
  }
  if (a.out_states) xa_step_row<T>(a.out_states, i, ob)[e] = old;
  if (a.out_new_states) xa_step_row<T>(a.out_new_states, i, ob)[e] = nw;
  st[e] = post;
}

// The scalars of env i's step (reward r, done d): ring action / reward / done and count,
// the out_* rows at out_ld, the finished episode's return, ep_return and done.
XA_DEV void xa_step_scalars(const XaReplayStepArgs& a, int i, int64_t slot, float r, float d) {
  float ep = a.ep_return[i] + r;
  if (slot >= 0) {
    const int64_t cnt = a.ring_count[i];
    a.ring_count[i] = a.ring_kind == XA_RING_RB2 ? (cnt < a.capacity ? cnt + 1 : cnt) : cnt + 1;
    const uint8_t* src = (const uint8_t*)a.actions + (int64_t)i * a.act_bytes;
    uint8_t* dst = (uint8_t*)a.ring_actions + slot * a.act_bytes;
    for (int64_t b = 0; b < a.act_bytes; ++b) dst[b] = src[b];
    a.ring_rewards[slot] = r;
    a.ring_dones[slot] = d;
  }
  const int64_t o = (int64_t)i * (a.out_ld > 0 ? a.out_ld : 1);
  if (a.out_rewards) a.out_rewards[o] = r;
  if (a.out_dones) a.out_dones[o] = d;
  if (a.done_epret) a.done_epret[o] = d != 0.0f ? ep : 0.0f;
  if (d != 0.0f) ep = 0.0f;
  a.ep_return[i] = ep;
  a.done[i] = d;
}
