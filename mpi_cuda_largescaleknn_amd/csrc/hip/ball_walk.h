// The ball walk shared by the neighbour lists (knn_neighbors.hip), the radius searches
// (radius.hip, radius_var.hip), the clustering (cluster.hip), their periodic forms
// (periodic.hip, knn_periodic.hip) and the profiles (radius_profile.hip), with the pieces
// their exactness arguments rest on, each written once: the bucket scan, the span of a node,
// the far-corner distance, the cover of an accepted node and the statistics.
// One wave owns 64 curve-consecutive sorted queries (lane = query)
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

// Sorted positions [p0, p1) of `node` at level lvl (its buckets, the last one clipped at n).
__device__ __forceinline__ void node_span(const lsk_tree_view &T, uint32_t node, int32_t lvl, int64_t &p0,
                                          int64_t &p1) {
  const int32_t span_lg = T.depth - lvl;
  const int64_t first = ((int64_t)node - ((int64_t)1 << lvl)) << span_lg;
  p0 = first * kBucket;
  p1 = min(T.n, (first + ((int64_t)1 << span_lg)) * kBucket);
}

// The canonical dist2 from (qx, qy, qz) to the farthest corner of a box. Per-axis float
// differences, squares and fma are monotone, so no finite point inside the box has a larger
// computed d² (knn_exact.hip::count_tree carries the same argument about its own centre).
__device__ __forceinline__ float far_dist2(float qx, float qy, float qz, const float4 &lo4, const float4 &hi4) {
  const float fx = fmaxf(fabsf(lo4.x - qx), fabsf(hi4.x - qx));
  const float fy = fmaxf(fabsf(lo4.y - qy), fabsf(hi4.y - qy));
  const float fz = fmaxf(fabsf(lo4.z - qz), fabsf(hi4.z - qz));
  return dist2(fx, fy, fz);
}

// "This lane took a whole node when the stack stood at sp." The walk pops a node, then pushes
// its descendants above the place it was popped from, so everything popped while the stack is
// at least that high lies inside the taken node and the lane ignores it; the first pop below
// ends the cover. on_node calls pop(sp) first, then asks on(); take(sp) starts a cover.
struct Cover {
  bool is = false;
  uint32_t at = 0;
  __device__ __forceinline__ void pop(uint32_t sp) {
    if (is && sp < at) is = false;
  }
  __device__ __forceinline__ void take(uint32_t sp) {
    is = true;
    at = sp;
  }
  __device__ __forceinline__ bool on() const { return is; }
  __device__ __forceinline__ void clear() { is = false; }  // a new walk (the next image)
};

// The per-point columns that travel with a bucket's points through scan_bucket: load(pi) reads
// the lane's own point's value, get(j) broadcasts that of point j to the wave. NoCol is no
// column at all: no register, no instruction.
struct NoCol {
  struct value {};
  __device__ __forceinline__ void load(int64_t) {}
  __device__ __forceinline__ value get(int) const { return {}; }
};
// An integer column of up to 32 bits, widened (the input rows perm[pos], the core flags).
// !kOn: the column of a kernel form that has the value in its code but never reads it (the
// ids of a count walk): the constant 0, as free as NoCol.
template <class T, bool kOn = true>
struct Col {
  static_assert(sizeof(T) <= 4, "one readlane per value");
  const T *p;
  uint32_t r = 0;
  __device__ __forceinline__ void load(int64_t pi) {
    if (kOn) r = (uint32_t)p[pi];
  }
  __device__ __forceinline__ uint32_t get(int j) const {
    return kOn ? (uint32_t)__builtin_amdgcn_readlane((int)r, j) : 0u;
  }
};
struct FloatCol {  // (the per-point cutoffs)
  const float *p;
  float r = 0.f;
  __device__ __forceinline__ void load(int64_t pi) { r = p[pi]; }
  __device__ __forceinline__ float get(int j) const { return readlane_f(r, j); }
};
struct WeightCol {  // int64 weights as wrapping unsigned: two readlanes
  const int64_t *p;
  uint32_t lo = 0, hi = 0;
  __device__ __forceinline__ void load(int64_t pi) {
    const unsigned long long w = (unsigned long long)p[pi];
    lo = (uint32_t)w;
    hi = (uint32_t)(w >> 32);
  }
  __device__ __forceinline__ unsigned long long get(int j) const {
    const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)lo, j);
    const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)hi, j);
    return ((unsigned long long)h << 32) | (unsigned long long)l;
  }
};

// The open-box difference of scan_bucket: the canonical d² of Q - p; every candidate is `mine`.
// (periodic_image.h has the periodic one.)
struct OpenDiff {
  __device__ __forceinline__ float operator()(const GroupQuery &Q, float x, float y, float z, bool &mine) const {
    mine = true;
    return dist2(Q.x - x, Q.y - y, Q.z - z);
  }
};

// What scan_bucket hands to its functor per candidate: d² under the scan's difference, whether
// the pair belongs to the walk's image (open box: always), the candidate's sorted position and
// the values of the two columns.
template <class A, class B>
struct Candidate {
  float d2;
  bool mine;
  uint32_t pos;
  A a;
  B b;
};

// Scan bucket `node` (level T.depth): its points, and the columns `ca` / `cb` beside them, are
// loaded one per lane and broadcast in order; a lane with `use` set calls cand(c, use) with
// the Candidate c of each, and may clear `use` there to stop. Returns the bucket's point
// count. The only load-and-broadcast loop of the walks: what differs between them is `diff`
// and the columns.
template <class Diff, class ColA, class ColB, class Cand>
__device__ __forceinline__ int scan_bucket(const lsk_tree_view &T, uint32_t node, int lane, const GroupQuery &Q,
                                           const Diff &diff, ColA ca, ColB cb, bool &use, Cand cand) {
  const int64_t base = ((int64_t)node - ((int64_t)1 << T.depth)) * kBucket;
  if (base >= T.n) return 0;
  const int cnt = (int)min((int64_t)kBucket, T.n - base);
  const int64_t pi = base + lane;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (lane < cnt) {
    px = T.pts[3 * pi];
    py = T.pts[3 * pi + 1];
    pz = T.pts[3 * pi + 2];
    ca.load(pi);
    cb.load(pi);
  }
  for (int j = 0; j < cnt; j++) {
    const float x = readlane_f(px, j), y = readlane_f(py, j), z = readlane_f(pz, j);
    auto a = ca.get(j);
    auto b = cb.get(j);
    if (use) {
      bool mine;
      const float d2 = diff(Q, x, y, z, mine);
      cand(Candidate<decltype(a), decltype(b)>{d2, mine, (uint32_t)(base + j), a, b}, use);
    }
  }
  return cnt;
}

// The statistics of a walk, added to stats[0 .. 3] (and, kFifth, stats[4]) by one lane per
// wave: distance evaluations and whole-box acceptances are per lane and summed here, as is
// `fifth` (the CAS retries of the clustering hooks; a wave-uniform count, the image walks of
// the periodic kernels, comes from lane 0 alone); nodes popped and buckets scanned are
// wave-uniform. stats may be null.
template <bool kFifth>
__device__ __forceinline__ void add_stats(unsigned long long *stats, int lane, uint32_t evals, uint32_t nodes,
                                          uint32_t buckets, uint32_t accepts, uint32_t fifth = 0u) {
  if (!stats) return;
  const uint32_t e = wave_sum(evals), a = wave_sum(accepts), f = kFifth ? wave_sum(fifth) : 0u;
  if (lane == 0) {
    atomicAdd(&stats[0], (unsigned long long)e);
    atomicAdd(&stats[1], (unsigned long long)nodes);
    atomicAdd(&stats[2], (unsigned long long)buckets);
    atomicAdd(&stats[3], (unsigned long long)a);
    if (kFifth) atomicAdd(&stats[4], (unsigned long long)f);
  }
}

// The DFS. Every popped bucket, and with kTestInner every popped inner node too, has its own
// box loaded and handed to on_node(node, lvl, sp, lo4, hi4), which returns whether the lane
// needs the node (`use`); a node no lane needs is dropped. Inner nodes are then expanded with
// `keep` (see expand), buckets go to on_bucket(node, use). Without kTestInner an inner
// node's own box is never loaded: its descendants were culled against the group already.
// ball_walk_from walks the subtree of `root` alone (a node that covers at least one bucket):
// the stack argument of walk_stack holds for it a fortiori, a subtree being no deeper than
// the tree. mst.hip walks the siblings of a bucket's ancestors one after the other with it.
template <bool kTestInner, class Keep, class OnNode, class OnBucket>
__device__ __forceinline__ void ball_walk_from(const lsk_tree_view &T, uint32_t *stk, int lane, uint32_t root,
                                               Keep keep, OnNode on_node, OnBucket on_bucket) {
  const int32_t depth = T.depth;
  const int64_t nb = (T.n + kBucket - 1) / kBucket;
  const float4 *nodes = (const float4 *)T.nodes;
  uint32_t sp = 1;
  if (lane == 0) stk[0] = root;
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

template <bool kTestInner, class Keep, class OnNode, class OnBucket>
__device__ __forceinline__ void ball_walk(const lsk_tree_view &T, uint32_t *stk, int lane, Keep keep,
                                          OnNode on_node, OnBucket on_bucket) {
  ball_walk_from<kTestInner>(T, stk, lane, 1u, keep, on_node, on_bucket);
}

}  // namespace lsk
