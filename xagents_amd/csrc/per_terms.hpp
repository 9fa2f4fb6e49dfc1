// The arithmetic of prioritized experience replay (Schaul et al., arXiv:1511.05952), stated
// once for per.hip's kernels: the 64-ary sum tree's shape and node sum, the stratified
// target, the descent's child choice, the importance weight and the leaf a TD error becomes.
// tests/per_ref.py restates these lines in float64.
#pragma once
#include "xa_common.hpp"

namespace xa_per {

constexpr int kFan = 64;        // children per node: one wave lane each
constexpr int kMaxLevels = 8;   // 64^8 leaves: more than an int64 slot count can name

// The tree over L leaves. Level 0 is the float leaf array (priority^alpha, 0 for a slot
// never written); level l >= 1 has n[l] = ceil(n[l-1] / 64) double nodes, stored one level
// after the other in ONE double array at off[l] (level 1 first), until a level has a single
// node, the root. A child index past its level's end (the ragged last node) counts as 0.
struct Shape {
  int levels;                 // internal levels: the root is level `levels`
  int64_t n[kMaxLevels + 1];  // n[0] = L
  int64_t off[kMaxLevels + 1];
};

__host__ __device__ inline Shape shape_of(int64_t n_leaves) {
  Shape s;
  s.n[0] = n_leaves;
  s.off[0] = 0;
  s.levels = 0;
  int64_t n = n_leaves, off = 0;
  do {
    n = (n + kFan - 1) / kFan;
    ++s.levels;
    s.n[s.levels] = n;
    s.off[s.levels] = off;
    off += n;
  } while (n > 1 && s.levels < kMaxLevels);
  return s;
}

__host__ __device__ inline int64_t node_count(int64_t n_leaves) {
  const Shape s = shape_of(n_leaves);
  return s.off[s.levels] + 1;
}

// child `lane` of node k of level l (l >= 1), as a double; 0 past the end of level l - 1
XA_DEV double child(const Shape& s, const float* leaves, const double* nodes, int l, int64_t k,
                    int lane) {
  const int64_t c = k * kFan + lane;
  if (c >= s.n[l - 1]) return 0.0;
  return l == 1 ? (double)leaves[c] : nodes[s.off[l - 1] + c];
}

// A node is always the sum of its 64 children in xa_wave_sum_f64's order (lane i holds
// child i), never its old value plus a delta: no atomics, no drift, and two writers of one
// node store the same bits.
XA_DEV double node_sum(double child_of_lane) { return xa_wave_sum_f64(child_of_lane); }

// stratified target of sample j of B: ((j + u) / B) root, u in [0, 1)
XA_DEV double target(int j, float u, int B, double root) {
  return ((double)j + (double)u) / (double)B * root;
}

// uniform of sample j at draw `ctr`: xa_u01 of Philox4x32-10 at (j, 0, ctr), key seed
XA_DEV float uniform(int j, uint64_t ctr, uint64_t seed) {
  const xa_u4 r = xa_philox((uint32_t)j, 0u, (uint32_t)ctr, (uint32_t)(ctr >> 32),
                            (uint32_t)seed, (uint32_t)(seed >> 32));
  return xa_u01(r.x);
}

// inclusive prefix sums over the wave's lanes, f64 (Hillis-Steele: lane i adds lane i - d,
// d = 1, 2, ..., 32)
XA_DEV double wave_prefix(double v, int lane) {
#pragma unroll
  for (int d = 1; d < kFan; d <<= 1) {
    const double up = __shfl_up(v, d, kFan);
    if (lane >= d) v = v + up;
  }
  return v;
}

// One descent step, wave-uniform: lane i holds child c_i and its inclusive prefix S_i. The
// chosen child is the first with t < S_i and c_i > 0; if rounding leaves none, the last with
// c_i > 0 (a child holding 0 is never entered, so a zero leaf is never returned while the
// root is > 0). t becomes t - S_{i-1}. Returns the child's lane (0 if every child is 0).
XA_DEV int descend(double c, double S, double& t) {
  const unsigned long long pos = __ballot(c > 0.0);
  const unsigned long long hit = __ballot(t < S && c > 0.0);
  int i = 0;
  if (hit)
    i = __ffsll((long long)hit) - 1;
  else if (pos)
    i = 63 - __clzll((long long)pos);
  const double before = __shfl(S, i > 0 ? i - 1 : 0, kFan);
  if (i > 0) t = t - before;
  return i;
}

// importance weight before the batch-max normalisation, f64: (N leaf / root)^(-beta)
XA_DEV double weight(int64_t n_stored, float leaf, double root, float beta) {
  return pow((double)n_stored * (double)leaf / root, -(double)beta);
}

// the priority a TD error becomes, and the leaf that stores it (already exponentiated)
XA_DEV float priority(float td_abs, float eps) { return td_abs + eps; }
XA_DEV float leaf_of(float priority, float alpha) { return powf(priority, alpha); }

}  // namespace xa_per
