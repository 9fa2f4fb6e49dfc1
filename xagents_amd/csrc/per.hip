// Prioritized experience replay on device: a 64-ary sum tree in HBM over the replay rings'
// global slots (env * cap + row), its stratified sampler and the priority updates. The
// arithmetic is per_terms.hpp's.
//
// Layout. Level 0 holds L = n_envs * cap leaves in float: priority^alpha already
// exponentiated, 0 for a slot never written. Level l >= 1 has ceil(n_{l-1} / 64) nodes in
// double, until a level has one node (the root); all internal levels live in ONE double array,
// level 1 first, each at its level offset (xa_per::shape_of). A missing child of the ragged
// last node counts as 0.
//
// A node is always recomputed from its 64 children -- lane i loads child i, the wave sums in
// xa_wave_sum_f64's order -- and never updated by a delta, so there are no atomics and no
// drift: two batch items that share an ancestor store the same bits. A leaf has one writer
// per launch: of the items that list one slot, the last stores it (their TD errors need not
// agree: SAC draws a next action per row).
//
// Mark, update and sample are ONE workgroup each (batches are tens to a few hundred items,
// the tree has 3-4 levels at a million leaves: latency-bound, like the TD3 / SAC row kernels).
// Between two levels stands level_barrier(): every wave first waits for its own global stores
// (s_waitcnt vmcnt(0): the barrier instruction itself waits for no counter, and at workgroup
// scope the compiler's fence emits none), then __syncthreads(). The waves of one workgroup
// run on one CU and read through the one vector L1 their stores went through, so behind the
// barrier they see the level below (no other workgroup reads the tree inside a launch; the
// next launch on the stream sees it through the kernel boundary). The tree is only ever
// loaded per lane (vector loads) through pointers the kernel also stores through, never
// through the scalar cache.
#include "../../include/xagents_hip.h"
#include "per_terms.hpp"
#include "xa_common.hpp"

namespace {

using xa_per::kFan;
using xa_per::Shape;

constexpr int kBlock = 256;  // the one workgroup of mark / update / sample
constexpr int kWaves = kBlock / kFan;

// this wave's global stores have completed, then the workgroup's barrier
XA_DEV void level_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// Every ancestor of items 0 .. n_items - 1 (slot_of(b): the item's leaf, < 0 or >= L: no
// item), level by level: wave w recomputes the level-l ancestors of items w, w + kWaves, ...
// Callers have stored the leaves; the barrier in front of each level publishes the level below.
template <typename SlotOf>
XA_DEV void recompute_ancestors(const Shape& s, float* leaves, double* nodes, int n_items,
                                SlotOf slot_of) {
  const int lane = threadIdx.x & (kFan - 1), wave = threadIdx.x / kFan;
  int64_t span = 1;  // leaves under one node of level l
  for (int l = 1; l <= s.levels; ++l) {
    level_barrier();
    span *= kFan;
    if (s.n[l] == 1) {
      // a one-node level (the root): once, whatever the items are
      if (wave == 0) {
        const double v = xa_per::node_sum(xa_per::child(s, leaves, nodes, l, 0, lane));
        if (lane == 0) nodes[s.off[l]] = v;
      }
      continue;
    }
    for (int b = wave; b < n_items; b += kWaves) {
      const int64_t slot = slot_of(b);  // wave-uniform
      if (slot < 0 || slot >= s.n[0]) continue;
      const int64_t k = slot / span;
      const double v = xa_per::node_sum(xa_per::child(s, leaves, nodes, l, k, lane));
      if (lane == 0) nodes[s.off[l] + k] = v;
    }
  }
}

// the slot env e's next append lands in (xa_step_ring_slot's rule; both ring kinds)
XA_DEV int64_t mark_slot(const int64_t* count, int e, int64_t cap) {
  const int64_t c = count[e];
  return c < 0 ? -1 : (int64_t)e * cap + c % cap;
}

__global__ __launch_bounds__(kBlock) void per_mark_kernel(Shape s, float* leaves, double* nodes,
                                                          const int64_t* count, int n_envs,
                                                          int64_t cap, const float* max_priority,
                                                          float alpha) {
  const float p = xa_per::leaf_of(max_priority[0], alpha);
  for (int e = threadIdx.x; e < n_envs; e += kBlock) {
    const int64_t slot = mark_slot(count, e, cap);
    if (slot >= 0 && slot < s.n[0]) leaves[slot] = p;
  }
  recompute_ancestors(s, leaves, nodes, n_envs,
                      [=](int e) { return mark_slot(count, e, cap); });
}

__global__ __launch_bounds__(kBlock) void per_update_kernel(Shape s, float* leaves,
                                                            double* nodes, const int64_t* slots,
                                                            const float* td_abs, int B,
                                                            float alpha, float eps,
                                                            float* max_priority) {
  __shared__ float wave_max[kWaves];
  float m = 0.0f;  // priorities are positive
  for (int b = threadIdx.x; b < B; b += kBlock) {
    const int64_t slot = slots[b];
    if (slot < 0 || slot >= s.n[0]) continue;
    const float p = xa_per::priority(td_abs[b], eps);
    m = fmaxf(m, p);
    // a slot listed more than once is stored by its LAST item alone (SAC's rows of one
    // transition draw different next actions, so their TD errors differ): one writer per
    // leaf, whatever order the threads run in
    bool last = true;
    for (int c = b + 1; c < B && last; ++c) last = slots[c] != slot;
    if (last) leaves[slot] = xa_per::leaf_of(p, alpha);
  }
  for (int d = 1; d < kFan; d <<= 1) m = fmaxf(m, __shfl_xor(m, d, kFan));
  if ((threadIdx.x & (kFan - 1)) == 0) wave_max[threadIdx.x / kFan] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) m = fmaxf(m, wave_max[w]);
    max_priority[0] = fmaxf(max_priority[0], m);
  }
  recompute_ancestors(s, leaves, nodes, B, [=](int b) { return slots[b]; });
}

// every node of level l from level l - 1: one wave per node (one launch per level)
__global__ __launch_bounds__(kBlock) void per_rebuild_level_kernel(Shape s, const float* leaves,
                                                                   double* nodes, int l) {
  const int lane = threadIdx.x & (kFan - 1), wave = threadIdx.x / kFan;
  for (int64_t k = (int64_t)blockIdx.x * kWaves + wave; k < s.n[l];
       k += (int64_t)gridDim.x * kWaves) {
    const double v = xa_per::node_sum(xa_per::child(s, leaves, nodes, l, k, lane));
    if (lane == 0) nodes[s.off[l] + k] = v;
  }
}

// Waves take samples w, w + kWaves, ...: the descent from the root, one node per level, lane
// i holding child i. Then, behind a barrier, the weights from the leaves the waves found.
__global__ __launch_bounds__(kBlock) void per_sample_kernel(
    Shape s, const float* leaves, const double* nodes, const int64_t* count, int n_envs,
    int64_t cap, int B, const float* u_in, const uint64_t* ctr, uint64_t seed, const float* beta,
    int64_t* slots, float* leaf_p, float* weights, float* u_out) {
  __shared__ long long n_part[kWaves];
  __shared__ double w_part[kWaves];
  const int lane = threadIdx.x & (kFan - 1), wave = threadIdx.x / kFan;
  const double root = nodes[s.off[s.levels]];
  // N = sum_e min(count[e], cap): the transitions stored
  long long n = 0;
  for (int e = threadIdx.x; e < n_envs; e += kBlock) {
    const int64_t c = count[e];
    n += c < cap ? (c > 0 ? c : 0) : cap;
  }
  for (int d = 1; d < kFan; d <<= 1) n += __shfl_xor(n, d, kFan);
  if (lane == 0) n_part[wave] = n;
  // (a given u_in draws nothing: the counter is not read either)
  const uint64_t c0 = (!u_in && ctr) ? ctr[0] : 0ull;
  for (int j = wave; j < B; j += kWaves) {
    const float u = u_in ? u_in[j] : xa_per::uniform(j, c0, seed);
    double t = xa_per::target(j, u, B, root);
    int64_t k = 0;
    for (int l = s.levels; l >= 1; --l) {
      const double c = xa_per::child(s, leaves, nodes, l, k, lane);
      const double S = xa_per::wave_prefix(c, lane);
      k = k * kFan + xa_per::descend(c, S, t);
    }
    if (k >= s.n[0]) k = s.n[0] - 1;  // (only an all-zero tree gets here)
    if (lane == 0) {
      slots[j] = k;
      leaf_p[j] = leaves[k];
      if (u_out) u_out[j] = u;
    }
  }
  level_barrier();  // leaf_p, stored by each wave's lane 0, is read by every thread below
  long long n_stored = 0;
  for (int w = 0; w < kWaves; ++w) n_stored += n_part[w];
  const float bt = beta[0];
  double m = 0.0;
  for (int j = threadIdx.x; j < B; j += kBlock)
    m = fmax(m, xa_per::weight(n_stored, leaf_p[j], root, bt));
  for (int d = 1; d < kFan; d <<= 1) m = fmax(m, __shfl_xor(m, d, kFan));
  if (lane == 0) w_part[wave] = m;
  __syncthreads();
  m = w_part[0];
  for (int w = 1; w < kWaves; ++w) m = fmax(m, w_part[w]);
  // the batch-max form: w_j / max_j w_j, rounded to f32 once
  for (int j = threadIdx.x; j < B; j += kBlock)
    weights[j] = (float)(xa_per::weight(n_stored, leaf_p[j], root, bt) / m);
}

}  // namespace

extern "C" size_t xa_per_tree_nodes(int64_t n_leaves) {
  return n_leaves > 0 ? (size_t)xa_per::node_count(n_leaves) : 0;
}

extern "C" int xa_per_rebuild(const float* leaves, double* nodes, int64_t n_leaves,
                              void* stream) {
  XA_CHECK_ARG(leaves && nodes && n_leaves > 0, "xa_per_rebuild: bad arguments");
  const Shape s = xa_per::shape_of(n_leaves);
  for (int l = 1; l <= s.levels; ++l) {
    const int64_t blocks = (s.n[l] + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(per_rebuild_level_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)),
                       dim3(kBlock), 0, (hipStream_t)stream, s, leaves, nodes, l);
    XA_CHECK_LAUNCH("xa_per_rebuild");
  }
  return 0;
}

extern "C" int xa_per_mark(float* leaves, double* nodes, int64_t n_leaves, const int64_t* count,
                           int n_envs, int64_t capacity, const float* max_priority, float alpha,
                           void* stream) {
  XA_CHECK_ARG(leaves && nodes && count && max_priority && n_envs > 0 && capacity > 0 &&
                   n_leaves == (int64_t)n_envs * capacity,
               "xa_per_mark: bad arguments (n_leaves is n_envs * capacity)");
  hipLaunchKernelGGL(per_mark_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream,
                     xa_per::shape_of(n_leaves), leaves, nodes, count, n_envs, capacity,
                     max_priority, alpha);
  XA_CHECK_LAUNCH("xa_per_mark");
  return 0;
}

extern "C" int xa_per_sample(const float* leaves, const double* nodes, int64_t n_leaves,
                             const int64_t* count, int n_envs, int64_t capacity, int batch,
                             const float* u_in, const uint64_t* rng_counter, uint64_t seed,
                             const float* beta, int64_t* slots, float* leaf_p, float* weights,
                             float* u_out, void* stream) {
  XA_CHECK_ARG(leaves && nodes && count && beta && slots && leaf_p && weights && batch > 0 &&
                   n_envs > 0 && capacity > 0 && n_leaves == (int64_t)n_envs * capacity,
               "xa_per_sample: bad arguments (n_leaves is n_envs * capacity)");
  XA_CHECK_ARG(u_in || rng_counter, "xa_per_sample: a draw needs rng_counter (or u_in)");
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream,
                     xa_per::shape_of(n_leaves), leaves, nodes, count, n_envs, capacity, batch,
                     u_in, rng_counter, seed, beta, slots, leaf_p, weights, u_out);
  XA_CHECK_LAUNCH("xa_per_sample");
  return 0;
}

extern "C" int xa_per_update(float* leaves, double* nodes, int64_t n_leaves, const int64_t* slots,
                             const float* td_abs, int batch, float alpha, float eps,
                             float* max_priority, void* stream) {
  XA_CHECK_ARG(leaves && nodes && slots && td_abs && max_priority && n_leaves > 0 && batch > 0,
               "xa_per_update: bad arguments");
  hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream,
                     xa_per::shape_of(n_leaves), leaves, nodes, slots, td_abs, batch, alpha, eps,
                     max_priority);
  XA_CHECK_LAUNCH("xa_per_update");
  return 0;
}
