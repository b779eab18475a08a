// The ball walk shared by the neighbour lists (knn_neighbors.hip) and the fixed-radius
// search (radius.hip): one wave owns 64 curve-consecutive sorted queries (lane = query)
// and walks the bucket tree once for the group. The DFS is wave-uniform with its stack in
// LDS; an inner node is expanded to its descendants kWalkStep levels down, one box per
// lane, and a bucket is scanned by the lanes whose own ball reaches it, its points
// broadcast one by one.
//
// A consumer supplies (ball_walk): `keep`, the cull of a descendant's box against the whole
// group; `on_node`, the per-lane decision on a popped node's own box; `on_bucket`, which as
// a rule calls scan_bucket with a per-candidate functor. Whether inner nodes are tested
// per lane (and their boxes loaded at all) is a compile-time choice.
#pragma once
#include "dev.h"

namespace lsk {

constexpr int kWalkStep = 6;  // levels per tree expansion (64 boxes, one per lane)

// DFS stack entries per wave for expansions of `step` levels: a tree is at most 30 deep, so
// <= ceil(30 / step) expansions leave 2^step - 1 siblings each, + 1; in whole 32-word rows.
constexpr int walk_stack(int step) {
  const int need = ((30 + step - 1) / step * ((1 << step) - 1) + 1 + 31) / 32 * 32;
  return need < 128 ? 128 : need;
}
constexpr int kWalkStack = walk_stack(kWalkStep);
static_assert(kWalkStack == 320, "the walk kernels' LDS footprint: 4 waves x 320 words");

__device__ __forceinline__ float readlane_f(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  const float inf = __builtin_inff();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}

// A node's box from the two float4 of its slot in the node array.
__device__ __forceinline__ box3f box_of(const float4 &lo4, const float4 &hi4) {
  return {{lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}};
}

// Expand `node` (level lvl < depth) to its descendants min(kWalkStep, depth - lvl) levels
// down: lane l < 2^step tests descendant l with `keep(lo4, hi4)` of its box; the kept ones
// (that cover at least one bucket < nb) are pushed. Returns the new stack pointer.
template <class Keep>
__device__ __forceinline__ uint32_t expand(const float4 *nodes, uint32_t node, int32_t lvl, int32_t depth,
                                           int64_t nb, uint32_t *stk, uint32_t sp, int lane, Keep keep) {
  const int32_t step = min(kWalkStep, depth - lvl);
  const uint32_t nc = 1u << step;
  const uint32_t child = (node << step) + (uint32_t)lane;
  bool need = false;
  if ((uint32_t)lane < nc) {
    const int32_t span_lg = depth - (lvl + step);
    const int64_t first = ((int64_t)child - ((int64_t)1 << (lvl + step))) << span_lg;
    if (first < nb) {
      const float4 lo4 = nodes[2 * child], hi4 = nodes[2 * child + 1];
      need = keep(lo4, hi4);
    }
  }
  const uint64_t m = __ballot(need);
  if (need) stk[sp + __popcll(m & ((1ull << lane) - 1ull))] = child;
  __builtin_amdgcn_wave_barrier();
  return sp + (uint32_t)__popcll(m);
}

// Lane's query of group g (g * kBucket < nq): sorted query qi, its coordinates and its row
// out_perm[qi] in query order. Lanes past nq are not `valid`; a query with a non-finite
// coordinate has d² = inf or NaN to every point, so it is not `finite` and has no neighbours.
struct GroupQuery {
  int64_t qi, row;
  float x, y, z;
  bool valid, finite;
};

__device__ __forceinline__ GroupQuery load_group(int64_t g, int lane, const float *qpts, const uint32_t *out_perm,
                                                 int64_t nq) {
  GroupQuery Q{g * kBucket + lane, 0, 0.f, 0.f, 0.f, false, false};
  Q.valid = Q.qi < nq;
  if (Q.valid) {
    Q.x = qpts[3 * Q.qi];
    Q.y = qpts[3 * Q.qi + 1];
    Q.z = qpts[3 * Q.qi + 2];
    Q.row = (int64_t)out_perm[Q.qi];
  }
  Q.finite = Q.valid && finite3(Q.x, Q.y, Q.z);
  return Q;
}

// Box of the group's `live` queries (uniform).
__device__ __forceinline__ box3f group_box(const GroupQuery &Q, bool live) {
  const float inf = __builtin_inff();
  return {{wave_min(live ? Q.x : inf), wave_min(live ? Q.y : inf), wave_min(live ? Q.z : inf)},
          {wave_max(live ? Q.x : -inf), wave_max(live ? Q.y : -inf), wave_max(live ? Q.z : -inf)}};
}

// Scan bucket `node` (level T.depth): its points (and, kIds, their input rows perm[pos]) are
// loaded one per lane and broadcast in order; a lane with `use` set calls cand(d2, id, use)
// for each, and may clear `use` there to stop. Returns the bucket's point count.
template <bool kIds, class Cand>
__device__ __forceinline__ int scan_bucket(const lsk_tree_view &T, const uint32_t *perm, uint32_t node, int lane,
                                           const GroupQuery &Q, bool &use, Cand cand) {
  const int64_t base = ((int64_t)node - ((int64_t)1 << T.depth)) * kBucket;
  if (base >= T.n) return 0;
  const int cnt = (int)min((int64_t)kBucket, T.n - base);
  const int64_t pi = base + lane;
  float px = 0.f, py = 0.f, pz = 0.f;
  uint32_t pid = 0;
  if (lane < cnt) {
    px = T.pts[3 * pi];
    py = T.pts[3 * pi + 1];
    pz = T.pts[3 * pi + 2];
    if (kIds) pid = perm[pi];
  }
  for (int j = 0; j < cnt; j++) {
    const float x = readlane_f(px, j), y = readlane_f(py, j), z = readlane_f(pz, j);
    uint32_t id = 0;
    if (kIds) id = (uint32_t)__builtin_amdgcn_readlane((int)pid, j);
    if (use) cand(dist2(Q.x - x, Q.y - y, Q.z - z), id, use);
  }
  return cnt;
}

// The DFS. Every popped bucket, and with kTestInner every popped inner node too, has its own
// box loaded and handed to on_node(node, lvl, sp, lo4, hi4), which returns whether the lane
// needs the node (`use`); a node no lane needs is dropped. Inner nodes are then expanded with
// `keep` (see expand), buckets go to on_bucket(node, use). Without kTestInner an inner
// node's own box is never loaded: its descendants were culled against the group already.
template <bool kTestInner, class Keep, class OnNode, class OnBucket>
__device__ __forceinline__ void ball_walk(const lsk_tree_view &T, uint32_t *stk, int lane, Keep keep,
                                          OnNode on_node, OnBucket on_bucket) {
  const int32_t depth = T.depth;
  const int64_t nb = (T.n + kBucket - 1) / kBucket;
  const float4 *nodes = (const float4 *)T.nodes;
  uint32_t sp = 1;
  if (lane == 0) stk[0] = 1u;
  __builtin_amdgcn_wave_barrier();
  while (sp > 0) {
    sp--;
    const uint32_t node = uniform(stk[sp]);
    const int32_t lvl = 31 - __clz(node);
    const bool inner = lvl < depth;
    bool use = true;
    if (kTestInner || !inner) {
      const float4 lo4 = nodes[2 * node], hi4 = nodes[2 * node + 1];
      use = on_node(node, lvl, sp, lo4, hi4);
      if (!__ballot(use)) continue;
    }
    if (inner)
      sp = expand(nodes, node, lvl, depth, nb, stk, sp, lane, keep);
    else
      on_bucket(node, use);
  }
}

}  // namespace lsk
