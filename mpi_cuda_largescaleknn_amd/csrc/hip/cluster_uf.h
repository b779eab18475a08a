// The lock-free union-find and the small helpers that the clustering walks share: cluster.hip
// (open box) and periodic.hip (periodic box) link the same forest over the sorted positions
// with the same invariants (cluster.hip states them under "unite").
#pragma once
#include "ball_walk.h"

namespace lsk {

// The Cover of a hook walk. Besides the node a lane is done with (`cov`), the clique node it is
// inside and needs one hit from (`one`): entered where its far corner was not below the
// cutoff, so the lane descends, and its first hit covers the rest of that clique's subtree.
struct CliqueCover {
  Cover cov, one;
  __device__ __forceinline__ void pop(uint32_t sp) {
    cov.pop(sp);
    one.pop(sp);
  }
  __device__ __forceinline__ void enter(uint32_t sp) {
    if (!one.on()) one.take(sp);
  }
  // a hit at sp: inside a clique entered before, all of that clique is covered
  __device__ __forceinline__ void hit(uint32_t sp) {
    cov.take(one.on() ? one.at : sp);
    one.clear();
  }
  __device__ __forceinline__ void clear() {
    cov.clear();
    one.clear();
  }
};

__device__ __forceinline__ bool tight(const float4 &lo4, const float4 &hi4, float cut2) {
  return dist2(hi4.x - lo4.x, hi4.y - lo4.y, hi4.z - lo4.z) < cut2;
}

__device__ __forceinline__ bool all_core(const int32_t *cpre, int64_t p0, int64_t p1) {
  return p1 > p0 && (int64_t)(cpre[p1] - cpre[p0]) == p1 - p0;
}

__device__ __forceinline__ uint32_t hint(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A root of x's component as far as the hints tell, with path halving (atomicMin: parent[x]
// only ever decreases, and only for an x that is no root).
__device__ __forceinline__ uint32_t find(uint32_t *parent, uint32_t x, uint32_t n, bool &bad) {
  for (uint32_t steps = 0;; steps++) {
    const uint32_t p = hint(parent + x);
    if (p == x) return x;
    if (p > x || steps > n) {  // (never: a parent lies below its child, so a chain ends within n steps)
      bad = true;
      return x;
    }
    const uint32_t g = hint(parent + p);
    if (g == p) return p;
    if (g > p) {
      bad = true;
      return x;
    }
    atomicMin(parent + x, g);
    x = g;
  }
}

// Links the components of the lane's own point (rq: a position of it, kept as low as the lane
// has seen) and of b.
__device__ __forceinline__ void unite(uint32_t *parent, uint32_t &rq, uint32_t b, uint32_t n, bool &bad,
                                      uint32_t &retries) {
  uint32_t ra = find(parent, rq, n, bad), rb = find(parent, b, n, bad);
  while (ra != rb && !bad) {
    const uint32_t hi = max(ra, rb), lo = min(ra, rb);
    const uint32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) {  // hooked
      ra = rb = lo;
      break;
    }
    retries++;  // hi was hooked meanwhile: old < hi is its parent
    ra = find(parent, old, n, bad);
    rb = lo;
  }
  rq = min(ra, rb);
}

// The lane's point of bucket g: a GroupQuery whose row is the sorted position itself.
__device__ __forceinline__ GroupQuery load_own(const lsk_tree_view &T, int64_t g, int lane) {
  GroupQuery Q{g * kBucket + lane, 0, 0.f, 0.f, 0.f, false, false};
  Q.valid = Q.qi < T.n;
  if (Q.valid) {
    Q.x = T.pts[3 * Q.qi];
    Q.y = T.pts[3 * Q.qi + 1];
    Q.z = T.pts[3 * Q.qi + 2];
    Q.row = Q.qi;
  }
  Q.finite = Q.valid && finite3(Q.x, Q.y, Q.z);
  return Q;
}

}  // namespace lsk
