// Periodic boundaries for the radius search (radius.hip, radius_var.hip gather) and the
// density clustering (cluster.hip): the same walks over the same open-box index, with the
// distance of a pair replaced by the minimum image of its difference.
//
// The contract. A period is (Lx, Ly, Lz), each > 0, +inf = open axis. Per axis, in float32:
//     d = q - p;  h = 0.5f * L;  if (d > h) d = d - L;  else if (d < -h) d = d + L;
// and pd2 = dist2(dx, dy, dz). fl(q - p) = -fl(p - q) and the branches mirror each other, so
// pd2(q, p) and pd2(p, q) have the same bits: the link relation is symmetric. The branches
// taken are the pair's wrap vector w(q, p) in {-1, 0, +1}^3 (d > h: -1, the query moves down
// by L; d < -h: +1), and w(p, q) = -w(q, p). Membership is pd2 < cut2, strict. L = inf never
// wraps (no comparison with +-inf holds for a finite d), so an open period gives the results
// of the open-box kernels bit for bit. Required by the callers: cut2 <= fl(h * h) on every
// finite axis.
//
// The image loop. A wave (64 queries, lane = query) walks the tree once per image shift s in
// {-1, 0, +1}^3 that some pair of (a live query of the group, a point of the root box) can
// take: s_a = -1 only if fl(max q_a - root.lo_a) > h_a, s_a = +1 only if fl(min q_a -
// root.hi_a) < -h_a (float subtraction is monotone, so no pair's fl(q_a - p_a) passes h_a when
// the extreme one does not); an open axis is only 0. Interior groups walk one image, face,
// edge and corner groups 2, 4 and 8.
//
// Exactly once. In image s a candidate counts iff w(q, p) == s and pd2 < cut2. A pair has one
// wrap vector, so it counts in one image, whatever the rounding. The candidate test alone
// decides; everything else only culls.
//
// The cull is conservative (proof). Boxes are tested against the shifted query range,
// fl(q + s L), by the gaps of box_box_dist2 / box_dist2; on an axis with s_a = 0 that is the
// open-box argument (monotone float differences: the gap is <= |fl(q - p)| for every p in the
// box). On a shifted axis take s_a = -1 (+1 mirrors) and u = 2^-24. The candidate value is D =
// fl(fl(q - p) - L) with |D - (q - p - L)| <= u |q - p| (1 + u) + u |q - p - L|. The gap G
// is, by monotonicity in the box corners, at most fl(fl(q - L) - p) or fl(p - fl(q - L)) of
// the pair itself, which differs from |q - L - p| by at most u |q - L| + u |q - L - p| (1 +
// u). Together G <= |D| + u (4 |q| + 3 |p| + 3 L)(1 + u). The gap is therefore reduced by e_a
// = 2^-21 (max |q_a| + max |p_a| + L_a) = 8 u (...), maxima over the group box and the root
// box: after its own three roundings e_a still exceeds 4 u (...)(1 + u) by more than the u
// (|q| + |p| + L) that rounding G - e_a can add, so max(0, fl(G - e_a)) <= |D|. Squares and
// fma are monotone: the cull value is <= pd2 for every pair of the image inside the box.
// Culling may add candidates, never drop one.
//
// Whole-box acceptance (count walk) stays exact. A lane takes a node without visiting its
// points only if, on every axis, both corners take wrap branch s_a: fl(q - p) is monotone in
// p and each branch is an interval of d, so every point between the corners takes s_a too,
// i.e. all of the node belongs to this image for this lane. d -> fl(d -+ L) is monotone as
// well, so the largest |wrapped difference| is at a corner; the canonical dist2 of the
// per-axis larger one < cut2 then bounds every point's pd2. Otherwise the lane descends.
//
// Tight nodes need no wrap. A tight node (cluster.hip: canonical dist2 of its box diagonal <
// cut2) has extent a per axis with fl(a a) <= dist2(diagonal) < cut2 <= fl(h h), and fl(a a)
// < fl(h h) implies a < h: no pair inside wraps, pd2 is the open-box d², and the clique
// pre-linking of cluster_init_kernel holds unchanged.
#include "cluster_uf.h"
#include "periodic_image.h"

namespace {

using lsk::fbits;
using namespace lsk::periodic;

constexpr int kWaves = 4;           // waves per block, one query group each (as radius.hip)

struct PerRadArgs {
  lsk_tree_view T;
  const uint32_t *perm;      // sorted position -> input row (fill)
  const float *qpts;         // sorted queries
  int64_t nq;
  float cut2;                // the cutoff of every query, or
  const float *qcut2;        // kVarGather: [nq], query order
  float L[3];                // the period
  const uint32_t *out_perm;  // sorted query -> query row
  int32_t *counts;           // count: [nq], query order
  const int64_t *offsets;    // fill: [nq + 1], query order
  int32_t *out_idx;          // fill: [total]
  uint32_t *out_dist;        // fill: [total] pd2 bits until lsk_hip_radius_sort finalises them
  uint32_t *err;             // fill
  unsigned long long *stats; // count, optional [5]: the four of radius.hip, image walks
};

// The count (kFill = false) and fill walks of radius.hip (one cutoff) and of radius_var.hip's
// gather (kVarGather: the lane's own cutoff) under a period: the walk of those kernels, once
// per image.
template <bool kVarGather, bool kFill>
__global__ __launch_bounds__(kWaves * 64) void radius_periodic_walk_kernel(const PerRadArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= A.nq) return;  // (wave-uniform)
  const lsk::GroupQuery Q = lsk::load_group(g, lane, A.qpts, A.out_perm, A.nq);
  const int64_t row = Q.row;
  float cut2 = A.cut2;
  if (kVarGather) {
    cut2 = 0.f;
    if (Q.valid) cut2 = A.qcut2[row];
  }
  int64_t cur = 0, end = 0;
  if (kFill && Q.valid) {
    cur = A.offsets[row];
    end = A.offsets[row + 1];
  }
  const bool live = Q.finite && cut2 > 0.f;
  uint32_t count = 0;
  bool bad = false;
  lsk::Cover cov;  // count: the whole node the lane took
  uint32_t s_evals = 0, s_accepts = 0, s_nodes = 0, s_buckets = 0, s_images = 0;

  if (__ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    const float gmax = kVarGather ? lsk::wave_max(live ? cut2 : 0.f) : cut2;
    const lsk_tree_view &T = A.T;
    const Frame F = make_frame(T, A.L, gb);
    for (int im = 0; im < 27; im++) {  // (wave-uniform)
      Image I;
      if (!image_of(F.X, F.Y, F.Z, im, I)) continue;
      if (!(image_box_dist2(gb, F.rlo, F.rhi, I) < gmax)) continue;
      s_images++;
      cov.clear();
      lsk::ball_walk<true>(
          T, stk_all[wid], lane,
          [&](const float4 &lo4, const float4 &hi4) { return image_box_dist2(gb, lo4, hi4, I) < gmax; },
          [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
            s_nodes++;
            bool use = live && !bad && image_point_dist2(Q, lo4, hi4, I) < cut2;
            if (!kFill) {
              cov.pop(sp);
              use = use && !cov.on();
              if (use && box_inside(Q, lo4, hi4, F.X, F.Y, F.Z, I, cut2)) {
                // the node's points: its buckets, the last one clipped at n
                int64_t p0, p1;
                lsk::node_span(T, node, lvl, p0, p1);
                if (p1 > p0) count += (uint32_t)(p1 - p0);
                cov.take(sp);
                use = false;
                s_accepts++;
              }
            }
            return use;
          },
          [&](uint32_t node, bool use) {
            const bool evals = use;
            const int cnt = lsk::scan_bucket(
                T, node, lane, Q, ImageDiff{F, I}, lsk::Col<uint32_t, kFill>{A.perm}, lsk::NoCol{}, use,
                [&](const auto &c, bool &use) {
                  if (c.mine && c.d2 < cut2) {
                    if (!kFill) {
                      count++;
                    } else if (cur < end) {
                      A.out_idx[cur] = (int32_t)c.a;
                      A.out_dist[cur] = fbits(c.d2);
                      cur++;
                    } else {  // more than the count pass saw: stop appending
                      bad = true;
                      use = false;
                    }
                  }
                });
            if (cnt) s_buckets++;
            if (evals) s_evals += (uint32_t)cnt;
          });
    }
  }

  if (!kFill) {
    if (Q.valid) A.counts[row] = (int32_t)count;
    lsk::add_stats<true>(A.stats, lane, s_evals, s_nodes, s_buckets, s_accepts, lane == 0 ? s_images : 0u);
  } else if (Q.valid && (bad || cur != end)) {
    atomicAdd(A.err, 1u);
  }
}

struct PerClusterArgs {
  lsk_tree_view T;
  const uint32_t *perm;      // sorted position -> input row (border)
  const uint8_t *core;       // [n] core flags, sorted positions
  const int32_t *cpre;       // [n + 1] exclusive prefix sum of core (hook)
  float cut2;
  float L[3];                // the period
  int32_t half;              // hook: as cluster.hip
  uint32_t *parent;          // [n] (hook)
  const uint32_t *root;      // [n] (border)
  const uint32_t *minrow;    // [n] (border)
  int32_t *labels;           // [n] input order (border)
  uint32_t *err;             // hook
  unsigned long long *stats; // optional [5], as cluster.hip
};

// The hook walk of cluster.hip, once per image. The link relation is symmetric (pd2 and the
// mirrored wrap vector, above), so what that walk relies on carries over: `half` (the pair is
// left to the lane with the higher position, which meets it in image -s, and its cull cannot
// drop it), the one-hit mode inside a clique node (any hit of any image joins the clique's
// component), and a clique wave skipping buckets that are no clique (their core points are
// live in their own waves and take their hit in this wave's clique). cov / one are stack
// positions of one walk and start afresh in every image; a clique met again in another image
// costs one redundant unite.
__global__ __launch_bounds__(kWaves * 64) void cluster_periodic_hook_kernel(const PerClusterArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const lsk_tree_view &T = A.T;
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= T.n) return;  // (wave-uniform)
  const lsk::GroupQuery Q = lsk::load_own(T, g, lane);
  const float cut2 = A.cut2;
  const uint32_t n = (uint32_t)T.n;
  const uint32_t pos_q = (uint32_t)Q.qi;
  const bool live = Q.finite && cut2 > 0.f && A.core[Q.valid ? Q.qi : 0] != 0;
  if (!__ballot(live)) return;
  uint32_t rq = pos_q;  // a position of the lane's component, as low as the lane has seen
  bool bad = false;
  lsk::CliqueCover cc;
  uint32_t s_evals = 0, s_accepts = 0, s_nodes = 0, s_buckets = 0, s_retries = 0;
  const bool half = A.half != 0;

  const lsk::box3f gb = lsk::group_box(Q, live);
  const Frame F = make_frame(T, A.L, gb);
  // (wave-uniform) the wave's own bucket is a clique
  bool own_clique;
  {
    const uint32_t leaf = ((uint32_t)1 << T.depth) + (uint32_t)g;
    const float4 *nodes = (const float4 *)T.nodes;
    int64_t p0, p1;
    lsk::node_span(T, leaf, T.depth, p0, p1);
    own_clique = lsk::tight(nodes[2 * leaf], nodes[2 * leaf + 1], cut2) && lsk::all_core(A.cpre, p0, p1);
  }
  for (int im = 0; im < 27; im++) {  // (wave-uniform)
    Image I;
    if (!image_of(F.X, F.Y, F.Z, im, I)) continue;
    if (!(image_box_dist2(gb, F.rlo, F.rhi, I) < cut2)) continue;
    cc.clear();
    lsk::ball_walk<true>(
        T, stk_all[wid], lane,
        [&](const float4 &lo4, const float4 &hi4) { return image_box_dist2(gb, lo4, hi4, I) < cut2; },
        [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
          s_nodes++;
          cc.pop(sp);
          bool use = live && !bad && !cc.cov.on() && image_point_dist2(Q, lo4, hi4, I) < cut2;
          bool clique = false;  // (wave-uniform)
          int64_t p0 = 0, p1 = 0;
          if (__ballot(use) && lsk::tight(lo4, hi4, cut2)) {
            lsk::node_span(T, node, lvl, p0, p1);
            clique = lsk::all_core(A.cpre, p0, p1);
          }
          if (!clique) {
            if (own_clique && lvl == T.depth) use = false;
          } else if (use) {  // a clique node: one hit will do
            if (box_inside(Q, lo4, hi4, F.X, F.Y, F.Z, I, cut2)) {  // every point of it is linked to the lane's
              lsk::unite(A.parent, rq, (uint32_t)p0, n, bad, s_retries);
              cc.hit(sp);
              use = false;
              s_accepts++;
            } else {
              cc.enter(sp);
            }
          }
          return use;
        },
        [&](uint32_t node, bool use) {
          const bool evals = use;
          const int cnt = lsk::scan_bucket(
              T, node, lane, Q, ImageDiff{F, I}, lsk::Col<uint8_t>{A.core}, lsk::NoCol{}, use,
              [&](const auto &c, bool &use) {  // (c.a: the candidate's core flag)
                if (c.mine && c.d2 < cut2 && c.a) {
                  const bool one = cc.one.on();
                  if (c.pos != pos_q && (one || !half || c.pos < pos_q))
                    lsk::unite(A.parent, rq, c.pos, n, bad, s_retries);
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
  }
  if (bad) atomicAdd(A.err, 1u);
  lsk::add_stats<true>(A.stats, lane, s_evals, s_nodes, s_buckets, s_accepts, s_retries);
}

// The border walk of cluster.hip: the best (pd2 bits << 32 | input row) over all images.
__global__ __launch_bounds__(kWaves * 64) void cluster_periodic_border_kernel(const PerClusterArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const lsk_tree_view &T = A.T;
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= T.n) return;  // (wave-uniform)
  const lsk::GroupQuery Q = lsk::load_own(T, g, lane);
  const float cut2 = A.cut2;
  const bool live = Q.finite && cut2 > 0.f && A.core[Q.valid ? Q.qi : 0] == 0;
  if (!__ballot(live)) return;
  uint64_t best = ~0ull;  // (pd2 bits << 32 | input row) of the nearest core point so far
  uint32_t best_pos = 0;
  uint32_t s_evals = 0, s_nodes = 0, s_buckets = 0;
  const lsk::box3f gb = lsk::group_box(Q, live);
  const Frame F = make_frame(T, A.L, gb);
  for (int im = 0; im < 27; im++) {  // (wave-uniform)
    Image I;
    if (!image_of(F.X, F.Y, F.Z, im, I)) continue;
    if (!(image_box_dist2(gb, F.rlo, F.rhi, I) < cut2)) continue;
    lsk::ball_walk<true>(
        T, stk_all[wid], lane,
        [&](const float4 &lo4, const float4 &hi4) { return image_box_dist2(gb, lo4, hi4, I) < cut2; },
        [&](uint32_t, int32_t, uint32_t, const float4 &lo4, const float4 &hi4) {
          s_nodes++;
          // nothing of this image inside is nearer than the (slackened) box; a tie at the best
          // pd2 may still bring a lower row
          const float bd2 = image_point_dist2(Q, lo4, hi4, I);
          return live && bd2 < cut2 && fbits(bd2) <= (uint32_t)(best >> 32);
        },
        [&](uint32_t node, bool use) {
          const bool evals = use;
          const int cnt = lsk::scan_bucket(
              T, node, lane, Q, ImageDiff{F, I}, lsk::Col<uint32_t>{A.perm}, lsk::Col<uint8_t>{A.core}, use,
              [&](const auto &c, bool &) {
                if (c.mine && c.d2 < cut2 && c.b) {  // (c.a: input row, c.b: core flag)
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
  }
  if (live && best != ~0ull) A.labels[A.perm[Q.qi]] = (int32_t)A.minrow[A.root[best_pos]];
  lsk::add_stats<true>(A.stats, lane, s_evals, s_nodes, s_buckets, 0u, 0u);
}

// period: three values > 0 (+inf: open); bound: the largest squared cutoff, which must not
// exceed fl(h h) on a finite axis (negative: not checked here, the caller did).
int period_ok(const char *what, const float *period, float bound, float *L) {
  const float inf = __builtin_inff();
  for (int a = 0; a < 3; a++) {
    const float v = period ? period[a] : 0.f;
    if (!(v > 0.f)) {
      lsk::set_last_error(std::string(what) + ": period must be three values > 0 (+inf: open axis)");
      return 1;
    }
    const float h = 0.5f * v;
    if (v < inf && bound > h * h) {
      lsk::set_last_error(std::string(what) + ": the cutoff exceeds half the period of a finite axis");
      return 1;
    }
    L[a] = v;
  }
  return 0;
}

int per_rad_args(const char *what, const lsk_tree_view *tree, const float *qpts, int64_t nq, float cut2,
                 const float *qcut2, const float *period, const uint32_t *out_perm, PerRadArgs *A) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 32) || (!qcut2 && !(cut2 >= 0.f))) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)), "
                                            "0 <= nq < 2^32 or cut2 not >= 0");
    return 1;
  }
  *A = PerRadArgs{};
  if (period_ok(what, period, qcut2 ? -1.f : cut2, A->L)) return 1;
  if (nq > 0 && (!qpts || !out_perm)) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  A->T = *tree;
  A->qpts = qpts;
  A->nq = nq;
  A->cut2 = cut2;
  A->qcut2 = qcut2;
  A->out_perm = out_perm;
  return 0;
}

int per_cluster_args(const char *what, const lsk_tree_view *tree, const uint8_t *core, float cut2,
                     const float *period, PerClusterArgs *A) {
  if (!lsk_tree_ok(tree) || !(cut2 >= 0.f)) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)) "
                                            "or cut2 not >= 0");
    return 1;
  }
  *A = PerClusterArgs{};
  if (period_ok(what, period, cut2, A->L)) return 1;
  if (!core) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  A->T = *tree;
  A->core = core;
  A->cut2 = cut2;
  return 0;
}

}  // namespace

extern "C" int lsk_hip_radius_periodic_count(const lsk_tree_view *tree, const float *qpts, int64_t nq, float cut2,
                                             const float *qcut2, const float *period, const uint32_t *out_perm,
                                             int32_t *counts, unsigned long long *stats, void *stream) {
  PerRadArgs A;
  if (per_rad_args("radius_periodic_count", tree, qpts, nq, cut2, qcut2, period, out_perm, &A)) return 1;
  if (nq == 0) return 0;
  if (!counts) {
    lsk::set_last_error("radius_periodic_count: null argument");
    return 1;
  }
  A.counts = counts;
  A.stats = stats;
  const unsigned blocks = lsk_blocks((nq + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  if (qcut2)
    radius_periodic_walk_kernel<true, false><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  else
    radius_periodic_walk_kernel<false, false><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("radius_periodic_count");
  return 0;
}

extern "C" int lsk_hip_radius_periodic_fill(const lsk_tree_view *tree, const uint32_t *perm, const float *qpts,
                                            int64_t nq, float cut2, const float *qcut2, const float *period,
                                            const uint32_t *out_perm, const int64_t *offsets, int32_t *out_idx,
                                            float *out_dist, uint32_t *err, void *stream) {
  PerRadArgs A;
  if (per_rad_args("radius_periodic_fill", tree, qpts, nq, cut2, qcut2, period, out_perm, &A)) return 1;
  if (nq == 0) return 0;
  // (out_idx / out_dist may be null when every row is empty, as in lsk_hip_radius_fill)
  if (!perm || !offsets || !err) {
    lsk::set_last_error("radius_periodic_fill: null argument");
    return 1;
  }
  A.perm = perm;
  A.offsets = offsets;
  A.out_idx = out_idx;
  A.out_dist = (uint32_t *)out_dist;
  A.err = err;
  const unsigned blocks = lsk_blocks((nq + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  if (qcut2)
    radius_periodic_walk_kernel<true, true><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  else
    radius_periodic_walk_kernel<false, true><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("radius_periodic_fill");
  return 0;
}

extern "C" int lsk_hip_cluster_periodic_hook(const lsk_tree_view *tree, const uint8_t *core, const int32_t *cpre,
                                             float cut2, const float *period, int half, uint32_t *parent,
                                             uint32_t *err, unsigned long long *stats, void *stream) {
  PerClusterArgs A;
  if (per_cluster_args("cluster_periodic_hook", tree, core, cut2, period, &A)) return 1;
  if (!cpre || !parent || !err) {
    lsk::set_last_error("cluster_periodic_hook: null argument");
    return 1;
  }
  A.cpre = cpre;
  A.half = half;
  A.parent = parent;
  A.err = err;
  A.stats = stats;
  const unsigned blocks = lsk_blocks((A.T.n + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  cluster_periodic_hook_kernel<<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("cluster periodic hook");
  return 0;
}

extern "C" int lsk_hip_cluster_periodic_border(const lsk_tree_view *tree, const uint32_t *perm, const uint8_t *core,
                                               float cut2, const float *period, const uint32_t *root,
                                               const uint32_t *minrow, int32_t *labels, unsigned long long *stats,
                                               void *stream) {
  PerClusterArgs A;
  if (per_cluster_args("cluster_periodic_border", tree, core, cut2, period, &A)) return 1;
  if (!perm || !root || !minrow || !labels) {
    lsk::set_last_error("cluster_periodic_border: null argument");
    return 1;
  }
  A.perm = perm;
  A.root = root;
  A.minrow = minrow;
  A.labels = labels;
  A.stats = stats;
  const unsigned blocks = lsk_blocks((A.T.n + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  cluster_periodic_border_kernel<<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("cluster periodic border");
  return 0;
}
