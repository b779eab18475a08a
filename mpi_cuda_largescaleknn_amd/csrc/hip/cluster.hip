// Density clustering (friends-of-friends / DBSCAN labels) over one index, without storing a
// pair: connected components of the graph whose vertices are the core points and whose edges
// are the pairs with d² < cut2 (strict, the predicate of radius.hip), by a lock-free
// union-find over the sorted positions.
//
// Everything works in sorted positions: a wave owns one bucket of the index's own 64
// curve-consecutive points (lane = point), so the queries are T.pts themselves. The core
// flags come from lsk_hip_radius_count on the sorted points (the caller thresholds the
// counts with min_pts); `cpre` is their exclusive prefix sum, so "every point of a node is
// core" is two loads.
//
//  tight node   the canonical dist2 of its box diagonal (hi - lo per axis) is < cut2. Float
//               differences, squares and fma are monotone (radius.hip, count_tree), so no
//               pair of finite points inside has a larger computed d²: all are linked.
//  clique node  a tight node all of whose points are core: one component, whatever else
//               happens. (A tight node of >= min_pts points is one; so is a smaller one whose
//               points are core through neighbours outside it. Counting core flags instead
//               of the population also keeps a point with a NaN coordinate, which no box
//               sees and which is never core, out of every clique.) A parent that is a
//               clique makes both children cliques, so the clique nodes above a bucket are
//               a run of its ancestors.
//
//  1. cluster_init_kernel   parent[pos] = pos; a bucket that is a clique climbs to its highest
//     clique ancestor A and stores parent[pos] = first position of A: m exact copies cost
//     O(m), not O(m²).
//  2. cluster_hook_kernel   ball_walk<true> per bucket. A lane is live iff its point is
//     finite and core. Per candidate with d² < cut2 that is core: unite(pos_q, pos_p). Inside
//     a clique node a lane needs one hit only: if the node's far corner is < cut2 it unites
//     with the node's first position without a distance evaluation, otherwise it descends
//     and leaves the subtree after its first hit (CliqueCover of cluster_uf.h). A wave
//     whose own bucket is a clique skips every bucket that is none: a core point x of such a
//     bucket is live in its own wave, whose walk reaches this wave's clique (some point of it
//     is within cut2 of x) and takes a hit there, and all of the clique is linked already.
//     A dense core thus costs its own lanes no distance evaluation at all.
//  3. cluster_flatten_kernel (own launch: every hook is visible) root[pos] by following parent.
//  4. cluster_minrow_kernel  atomicMin(minrow[root[pos]], perm[pos]) over core points;
//     cluster_label_kernel   labels[perm[pos]] = minrow[root[pos]] for core points, -1 (or,
//     fof, the point's own row) for the others.
//  5. cluster_border_kernel  (min_pts > 1) live lanes are the finite non-core points; each
//     keeps the smallest (d² bits << 32 | input row) over core candidates with d² < cut2
//     and the candidate's sorted position beside it, and takes that candidate's label.
//
// unite — invariants:
//  * every value ever stored in parent[x] is <= x and lies in x's component (init: the first
//    position of a clique x belongs to; hook: the smaller of two roots just found linked;
//    halving: an ancestor of x);
//  * every linking decision is taken on the value an atomicCAS RETURNED. Loads of parent are
//    hints: they may be stale (another XCD's L2 inside a kernel), and a stale value is still
//    an ancestor that was valid once, so a walk over stale values ends at a smaller position
//    of the same component, and a CAS on a position that is no root any more fails and returns
//    its present parent;
//  * a failed CAS continues from the returned value, which is strictly below the position it
//    was tried on: every retry lowers a position, so unite terminates;
//  * no lane waits for another lane, wave or flag: no spin-wait, no lock, no barrier between
//    workgroups. A chain of parents strictly decreases, so a find ends within n steps; one
//    that does not bumps the error word and gives up (the host raises: a bug, no fallback).
// The components do not depend on the order in which the hooks land; the labels are taken
// from the components alone (smallest input row), so neither do they. unite, find and the
// node helpers live in cluster_uf.h, shared with the periodic walks of periodic.hip.
#include "cluster_uf.h"

namespace {

using lsk::all_core;
using lsk::fbits;
using lsk::load_own;
using lsk::node_span;
using lsk::tight;
using lsk::unite;

constexpr int kWaves = 4;  // waves per block, one bucket each (as radius.hip)

struct ClusterArgs {
  lsk_tree_view T;
  const uint32_t *perm;      // sorted position -> input row
  const uint8_t *core;       // [n] core flags, sorted positions
  const int32_t *cpre;       // [n + 1] exclusive prefix sum of core
  float cut2;
  int32_t half;              // hook: a bucket's candidates above the lane's own position are
                             // left to their own lanes (each pair united once)
  int32_t fof;               // label: a non-core point is a cluster of its own (min_pts = 1)
  uint32_t *parent;          // [n]
  uint32_t *root;            // [n]
  uint32_t *minrow;          // [n] smallest input row among a root's core points
  int32_t *labels;           // [n] input order
  uint32_t *err;
  unsigned long long *stats; // optional [5]: distance evaluations, nodes popped, buckets
                             // scanned, clique acceptances, CAS retries
};

__global__ __launch_bounds__(kWaves * 64) void cluster_init_kernel(const ClusterArgs A) {
  const int lane = lsk::lane_id();
  const lsk_tree_view &T = A.T;
  const int64_t nb = (T.n + lsk::kBucket - 1) / lsk::kBucket;
  const int64_t b = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= nb) return;  // (wave-uniform)
  const float4 *nodes = (const float4 *)T.nodes;
  auto clique = [&](uint32_t node, int32_t lvl, int64_t &p0) {
    int64_t p1;
    node_span(T, node, lvl, p0, p1);
    return tight(nodes[2 * node], nodes[2 * node + 1], A.cut2) && all_core(A.cpre, p0, p1);
  };
  uint32_t node = ((uint32_t)1 << T.depth) + (uint32_t)b;
  int32_t lvl = T.depth;
  const int64_t pos = b * lsk::kBucket + lane;
  int64_t p0, up0;
  uint32_t par = (uint32_t)pos;
  if (clique(node, lvl, p0)) {
    while (lvl > 0 && clique(node >> 1, lvl - 1, up0)) {
      node >>= 1;
      lvl--;
      p0 = up0;
    }
    par = (uint32_t)p0;
  }
  if (pos < T.n) {
    A.parent[pos] = par;
    A.minrow[pos] = 0xffffffffu;
  }
}

__global__ __launch_bounds__(kWaves * 64) void cluster_hook_kernel(const ClusterArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const lsk_tree_view &T = A.T;
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= T.n) return;  // (wave-uniform)
  const lsk::GroupQuery Q = load_own(T, g, lane);
  const float cut2 = A.cut2;
  const float qx = Q.x, qy = Q.y, qz = Q.z;
  const uint32_t n = (uint32_t)T.n;
  const uint32_t pos_q = (uint32_t)Q.qi;
  const bool live = Q.finite && cut2 > 0.f && A.core[Q.valid ? Q.qi : 0] != 0;
  if (!__ballot(live)) return;
  uint32_t rq = pos_q;  // a position of the lane's component, as low as the lane has seen
  bool bad = false;
  lsk::CliqueCover cc;  // the node the lane is done with; the clique it wants one hit from
  uint32_t s_evals = 0, s_accepts = 0, s_nodes = 0, s_buckets = 0, s_retries = 0;
  const bool half = A.half != 0;

  const lsk::box3f gb = lsk::group_box(Q, live);
  const lsk::vec3f q{qx, qy, qz};
  // (wave-uniform) the wave's own bucket is a clique
  bool own_clique;
  {
    const uint32_t leaf = ((uint32_t)1 << T.depth) + (uint32_t)g;
    const float4 *nodes = (const float4 *)T.nodes;
    int64_t p0, p1;
    node_span(T, leaf, T.depth, p0, p1);
    own_clique = tight(nodes[2 * leaf], nodes[2 * leaf + 1], cut2) && all_core(A.cpre, p0, p1);
  }
  lsk::ball_walk<true>(
      T, stk_all[wid], lane,
      [&](const float4 &lo4, const float4 &hi4) { return lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4)) < cut2; },
      [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
        s_nodes++;
        cc.pop(sp);
        bool use =
            live && !bad && !cc.cov.on() && lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}) < cut2;
        bool clique = false;  // (wave-uniform)
        int64_t p0 = 0, p1 = 0;
        if (__ballot(use) && tight(lo4, hi4, cut2)) {
          node_span(T, node, lvl, p0, p1);
          clique = all_core(A.cpre, p0, p1);
        }
        if (!clique) {
          // a bucket that is no clique, seen from a bucket that is one: left to that bucket's
          // own lanes, which walk too, meet this wave's clique and take their hit there
          if (own_clique && lvl == T.depth) use = false;
        } else {
          if (use) {  // a clique node: one hit will do
            if (lsk::far_dist2(qx, qy, qz, lo4, hi4) < cut2) {  // every point of it is linked to the lane's
              unite(A.parent, rq, (uint32_t)p0, n, bad, s_retries);
              cc.hit(sp);
              use = false;
              s_accepts++;
            } else {
              cc.enter(sp);
            }
          }
        }
        return use;
      },
      [&](uint32_t node, bool use) {
        const bool evals = use;
        const int cnt = lsk::scan_bucket(
            T, node, lane, Q, lsk::OpenDiff{}, lsk::Col<uint8_t>{A.core}, lsk::NoCol{}, use,
            [&](const auto &c, bool &use) {  // (c.a: the candidate's core flag)
              if (c.d2 < cut2 && c.a) {
                const bool one = cc.one.on();
                if (c.pos != pos_q && (one || !half || c.pos < pos_q)) unite(A.parent, rq, c.pos, n, bad, s_retries);
                if (one) {
                  cc.hit(0);
                  use = false;
                }
                if (bad) use = false;
              }
            });
        if (cnt) s_buckets++;
        if (evals) s_evals += (uint32_t)cnt;
      });
  if (bad) atomicAdd(A.err, 1u);
  lsk::add_stats<true>(A.stats, lane, s_evals, s_nodes, s_buckets, s_accepts, s_retries);
}

__global__ __launch_bounds__(256) void cluster_flatten_kernel(const ClusterArgs A) {
  const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= A.T.n) return;
  uint32_t x = (uint32_t)pos;
  if (A.core[pos]) {
    const uint32_t n = (uint32_t)A.T.n;
    uint32_t steps = 0;
    for (uint32_t p = A.parent[x]; p != x; p = A.parent[x]) {
      if (p > x || ++steps > n) {  // (never: see find)
        atomicAdd(A.err, 1u);
        break;
      }
      x = p;
    }
  }
  A.root[pos] = x;
}

// minrow[root] = the smallest input row of the root's core points. A wave whose core lanes
// share one root (a large component, a clique) sends one atomic; a lane whose row is not
// below the value already there (a hint: the value only decreases) sends none.
__global__ __launch_bounds__(256) void cluster_minrow_kernel(const ClusterArgs A) {
  const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = pos < A.T.n && A.core[pos < A.T.n ? pos : 0] != 0;
  if (!__ballot(act)) return;
  uint32_t r = 0, row = 0xffffffffu;
  if (act) {
    r = A.root[pos];
    row = A.perm[pos];
  }
  const uint64_t m = __ballot(act);
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r, (int)__builtin_ctzll(m));
  if (!__ballot(act && r != r0)) {
    uint32_t v = row;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    if (lsk::lane_id() == 0 && v < A.minrow[r0]) atomicMin(A.minrow + r0, v);
  } else if (act && row < A.minrow[r]) {
    atomicMin(A.minrow + r, row);
  }
}

__global__ __launch_bounds__(256) void cluster_label_kernel(const ClusterArgs A) {
  const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= A.T.n) return;
  const uint32_t row = A.perm[pos];
  int32_t label = A.fof ? (int32_t)row : -1;
  if (A.core[pos]) label = (int32_t)A.minrow[A.root[pos]];
  A.labels[row] = label;
}

__global__ __launch_bounds__(kWaves * 64) void cluster_border_kernel(const ClusterArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const lsk_tree_view &T = A.T;
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= T.n) return;  // (wave-uniform)
  const lsk::GroupQuery Q = load_own(T, g, lane);
  const float cut2 = A.cut2;
  const bool live = Q.finite && cut2 > 0.f && A.core[Q.valid ? Q.qi : 0] == 0;
  if (!__ballot(live)) return;
  uint64_t best = ~0ull;  // (d² bits << 32 | input row) of the nearest core point so far
  uint32_t best_pos = 0;
  uint32_t s_evals = 0, s_nodes = 0, s_buckets = 0;
  const lsk::box3f gb = lsk::group_box(Q, live);
  const lsk::vec3f q{Q.x, Q.y, Q.z};
  lsk::ball_walk<true>(
      T, stk_all[wid], lane,
      [&](const float4 &lo4, const float4 &hi4) { return lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4)) < cut2; },
      [&](uint32_t, int32_t, uint32_t, const float4 &lo4, const float4 &hi4) {
        s_nodes++;
        // nothing inside is nearer than the box; a tie at the best d² may still bring a lower row
        const float bd2 = lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z});
        return live && bd2 < cut2 && fbits(bd2) <= (uint32_t)(best >> 32);
      },
      [&](uint32_t node, bool use) {
        const bool evals = use;
        const int cnt = lsk::scan_bucket(T, node, lane, Q, lsk::OpenDiff{}, lsk::Col<uint32_t>{A.perm},
                                         lsk::Col<uint8_t>{A.core}, use, [&](const auto &c, bool &) {
                                           if (c.d2 < cut2 && c.b) {  // (c.a: input row, c.b: core flag)
                                             const uint64_t key = ((uint64_t)fbits(c.d2) << 32) | c.a;
                                             if (key < best) {
                                               best = key;
                                               best_pos = c.pos;
                                             }
                                           }
                                         });
        if (cnt) s_buckets++;
        if (evals) s_evals += (uint32_t)cnt;
      });
  if (live && best != ~0ull) A.labels[A.perm[Q.qi]] = (int32_t)A.minrow[A.root[best_pos]];
  lsk::add_stats<true>(A.stats, lane, s_evals, s_nodes, s_buckets, 0u, 0u);
}

int cluster_args(const char *what, const lsk_tree_view *tree, const uint8_t *core, float cut2, ClusterArgs *A) {
  if (!lsk_tree_ok(tree) || !(cut2 >= 0.f)) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)) "
                                            "or cut2 not >= 0");
    return 1;
  }
  if (!core) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  *A = ClusterArgs{};
  A->T = *tree;
  A->core = core;
  A->cut2 = cut2;
  return 0;
}

}  // namespace

extern "C" int lsk_hip_cluster_link(const lsk_tree_view *tree, const uint8_t *core, const int32_t *cpre, float cut2,
                                    int half, uint32_t *parent, uint32_t *minrow, uint32_t *err,
                                    unsigned long long *stats, void *stream) {
  ClusterArgs A;
  if (cluster_args("cluster_link", tree, core, cut2, &A)) return 1;
  if (!cpre || !parent || !minrow || !err) {
    lsk::set_last_error("cluster_link: null argument");
    return 1;
  }
  A.cpre = cpre;
  A.half = half;
  A.parent = parent;
  A.minrow = minrow;
  A.err = err;
  A.stats = stats;
  const unsigned blocks = lsk_blocks((A.T.n + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  cluster_init_kernel<<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("cluster init");
  cluster_hook_kernel<<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("cluster hook");
  return 0;
}

// The init pass of lsk_hip_cluster_link alone: the periodic hook (periodic.hip) runs after it.
extern "C" int lsk_hip_cluster_init(const lsk_tree_view *tree, const uint8_t *core, const int32_t *cpre, float cut2,
                                    uint32_t *parent, uint32_t *minrow, void *stream) {
  ClusterArgs A;
  if (cluster_args("cluster_init", tree, core, cut2, &A)) return 1;
  if (!cpre || !parent || !minrow) {
    lsk::set_last_error("cluster_init: null argument");
    return 1;
  }
  A.cpre = cpre;
  A.parent = parent;
  A.minrow = minrow;
  const unsigned blocks = lsk_blocks((A.T.n + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  cluster_init_kernel<<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("cluster init");
  return 0;
}

extern "C" int lsk_hip_cluster_label(const lsk_tree_view *tree, const uint32_t *perm, const uint8_t *core,
                                     const uint32_t *parent, int fof, uint32_t *root, uint32_t *minrow,
                                     int32_t *labels, uint32_t *err, void *stream) {
  ClusterArgs A;
  if (cluster_args("cluster_label", tree, core, 0.f, &A)) return 1;
  if (!perm || !parent || !root || !minrow || !labels || !err) {
    lsk::set_last_error("cluster_label: null argument");
    return 1;
  }
  A.perm = perm;
  A.parent = (uint32_t *)parent;
  A.fof = fof;
  A.root = root;
  A.minrow = minrow;
  A.labels = labels;
  A.err = err;
  const unsigned blocks = lsk_blocks(A.T.n, 256);
  hipStream_t st = (hipStream_t)stream;
  cluster_flatten_kernel<<<blocks, 256, 0, st>>>(A);
  LSK_CHECK_LAUNCH("cluster flatten");
  cluster_minrow_kernel<<<blocks, 256, 0, st>>>(A);
  LSK_CHECK_LAUNCH("cluster minrow");
  cluster_label_kernel<<<blocks, 256, 0, st>>>(A);
  LSK_CHECK_LAUNCH("cluster label");
  return 0;
}

extern "C" int lsk_hip_cluster_border(const lsk_tree_view *tree, const uint32_t *perm, const uint8_t *core,
                                      float cut2, const uint32_t *root, const uint32_t *minrow, int32_t *labels,
                                      unsigned long long *stats, void *stream) {
  ClusterArgs A;
  if (cluster_args("cluster_border", tree, core, cut2, &A)) return 1;
  if (!perm || !root || !minrow || !labels) {
    lsk::set_last_error("cluster_border: null argument");
    return 1;
  }
  A.perm = perm;
  A.root = (uint32_t *)root;
  A.minrow = (uint32_t *)minrow;
  A.labels = labels;
  A.stats = stats;
  const unsigned blocks = lsk_blocks((A.T.n + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  cluster_border_kernel<<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("cluster border");
  return 0;
}
