// The n-step transition a sampled replay slot stands for (xa_ring_gather_nstep, offpolicy.hip),
// stated once: how far the walk from the sampled slot may go, where it stops, and the f32
// order of its discounted reward sum and its bootstrap discount. The library is built with
// -ffp-contract=off, so the f32 operation order written here is the contract
// (tests/nstep_ref.py restates it in f32, bit for bit, and in float64).
//
// Ring: the deque kind only (XA_RING_DEQUE). One env's ring holds `capacity` slots; append
// number t (0-based) of the env lands on slot t mod capacity and count = appends so far, so
// consecutive slots (mod capacity) up to the newest are consecutive transitions of that env.
// For a sampled slot i of an env with counter c:
//   newest = (c - 1) mod capacity
//   avail  = ((newest - i) mod capacity) + 1      transitions from i to the newest, inclusive
//   m_max  = min(n_steps, avail)
//   L      = the first k in 0 .. m_max - 1 with dones[(i + k) mod capacity] != 0,
//            m_max - 1 if there is none;   m = L + 1 transitions are folded
// so the walk never crosses an episode end and never runs past the ring's head into the
// oldest entries. The folded transition is
//   (states[i], actions[i], R, dones[i + L], new_states[i + L]) with the discount gamma^m:
//   R = r_L; for k = L - 1 .. 0: R = r_k + gamma * R        (Horner, xa_nstep_returns' form)
//   g = gamma; m - 1 times: g = g * gamma
// n_steps = 1: L = 0, R = r_0's bits, g = gamma's bits.
#pragma once
#include <stdint.h>

#include "xa_common.hpp"

namespace xa_nstep {

constexpr int kMaxSteps = 64;  // one wave owns a walk: lane k holds step k

// slot j in [0, 2 capacity) back into the ring
XA_DEV int64_t wrap(int64_t j, int64_t capacity) { return j < capacity ? j : j - capacity; }

// m_max of slot i. An env that never appended (count <= 0) has no valid slot to sample; a walk
// there is one step long, which keeps every read inside the ring.
XA_DEV int max_steps(int64_t count, int64_t capacity, int64_t i, int n_steps) {
  if (count <= 0) return 1;
  const int64_t newest = (count - 1) % capacity;
  const int64_t back = newest - i;
  const int64_t avail = (back < 0 ? back + capacity : back) + 1;
  return (int)(avail < n_steps ? avail : n_steps);
}

// L from the wave's vote: bit k of done_mask is set iff k < m_max and step k's done != 0
XA_DEV int last_step(uint64_t done_mask, int m_max) {
  return done_mask ? __builtin_ctzll(done_mask) : m_max - 1;
}

// one Horner step of the reward sum, and the bootstrap discount of m folded transitions
XA_DEV float fold(float r, float gamma, float R) { return r + gamma * R; }
XA_DEV float discount(float gamma, int m) {
  float g = gamma;
  for (int t = 1; t < m; ++t) g = g * gamma;
  return g;
}

}  // namespace xa_nstep
