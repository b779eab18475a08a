// Two-sided radius search: a squared cutoff on the query (cq, gather) and on the indexed point
// (cp, scatter) at once. A pair is selected iff
//     either   d² < max(cq[q], cp[p])      (one ball reaches the other's centre)
//     both     d² < min(cq[q], cp[p])      (each ball reaches the other's centre)
// strictly, d² the canonical dist2 of q - p, or under a period pd2, the minimum image of
// periodic.hip with the pair's one wrap vector deciding the image. max and min are taken on
// float32 values that are never NaN, so the predicate is symmetric in its bits. Rows, offsets,
// the error word and the statistics are those of radius.hip; the rows are sorted and finalised
// by lsk_hip_radius_sort unchanged.
//
// One walk template over rule x {open, periodic} x {count, fill}: the walk of radius_var.hip
// with both of its sides live. It runs over the annotated node copy of the scatter search (lo.w
// = the largest cp below a node); a lane carries its own cq, and a candidate's cp travels beside
// its coordinates (FloatCol). Write rule(a, b) for max or min.
//
//  cull    a node N with annotation m = lo.w holds only points with cp <= m, and rule is monotone
//          in both arguments: for a lane, rule(cq, cp) <= rule(cq, m), and for the group, with
//          gmax the largest cq of its live lanes, <= rule(gmax, m). The box gap is a lower bound
//          of every d² inside (open: monotone float differences; periodic: the slackened gaps,
//          periodic.hip "The cull is conservative", which does not mention the threshold at
//          all). So gap >= rule(., m) implies d² >= rule(cq, cp) for every pair below N: culling
//          at that threshold drops no selected pair, under either rule. The same holds for the
//          image pre-cull against the root, whose lo.w is the largest cp of all.
//  live    either: the query is finite (a query with cq = 0 is still reached by points). both:
//          the query is finite and cq > 0 (min(0, .) = 0 selects nothing).
//  accept  (count, either) a lane takes a node whole when its far corner lies below its own cq
//          (periodic: box_inside): every point inside has d² <= far < cq <= max(cq, cp). Under
//          `both` there is no acceptance: it would need the smallest cp below the node.
//  pair    d² < rule(cq, cp), and under a period `mine`: the pair's wrap vector is the image's,
//          so it counts in one image (periodic.hip "Exactly once").
#include "periodic_image.h"

namespace {

using lsk::fbits;
using namespace lsk::periodic;

constexpr int kWaves = 4;  // waves per block, one query group each (as radius.hip)

struct ReachArgs {
  lsk_tree_view T;           // T.nodes is the annotated copy
  const uint32_t *perm;      // sorted position -> input row (fill)
  const float *qpts;         // sorted queries
  int64_t nq;
  const float *qcut2;        // [nq], query order
  const float *pcut2;        // [n], curve order
  float L[3];                // the period (periodic)
  const uint32_t *out_perm;  // sorted query -> query row
  int32_t *counts;           // count: [nq], query order
  const int64_t *offsets;    // fill: [nq + 1], query order
  int32_t *out_idx;          // fill: [total]
  uint32_t *out_dist;        // fill: [total] d² bits until lsk_hip_radius_sort finalises them
  uint32_t *err;             // fill
  unsigned long long *stats; // count, optional [4] (periodic: [5]), as radius.hip / periodic.hip
};

template <bool kBoth>
__device__ __forceinline__ float rule(float a, float b) {
  return kBoth ? fminf(a, b) : fmaxf(a, b);
}

template <bool kBoth, bool kPeriodic, bool kFill>
__global__ __launch_bounds__(kWaves * 64) void radius_reach_walk_kernel(const ReachArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= A.nq) return;  // (wave-uniform)
  const lsk::GroupQuery Q = lsk::load_group(g, lane, A.qpts, A.out_perm, A.nq);
  const int64_t row = Q.row;
  float cq = 0.f;
  if (Q.valid) cq = A.qcut2[row];
  int64_t cur = 0, end = 0;
  if (kFill && Q.valid) {
    cur = A.offsets[row];
    end = A.offsets[row + 1];
  }
  const bool live = Q.finite && (!kBoth || cq > 0.f);
  uint32_t count = 0;
  bool bad = false;
  lsk::Cover cov;  // either, count: the whole node the lane took
  uint32_t s_evals = 0, s_accepts = 0, s_nodes = 0, s_buckets = 0, s_images = 0;

  if (__ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    const float gmax = lsk::wave_max(live ? cq : 0.f);
    const lsk::vec3f q{Q.x, Q.y, Q.z};
    const lsk_tree_view &T = A.T;
    // one walk of the tree: the open box, or one image of the group
    auto walk = [&](const Frame &F, const Image &I) {
      lsk::ball_walk<true>(
          T, stk_all[wid], lane,
          [&](const float4 &lo4, const float4 &hi4) {
            const float gap = kPeriodic ? image_box_dist2(gb, lo4, hi4, I)
                                        : lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4));
            return gap < rule<kBoth>(gmax, lo4.w);
          },
          [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
            s_nodes++;
            const float gap = kPeriodic ? image_point_dist2(Q, lo4, hi4, I)
                                        : lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z});
            bool use = live && !bad && gap < rule<kBoth>(cq, lo4.w);
            if (!kBoth && !kFill) {
              cov.pop(sp);
              use = use && !cov.on();
              if (use && (kPeriodic ? box_inside(Q, lo4, hi4, F.X, F.Y, F.Z, I, cq)
                                    : lsk::far_dist2(Q.x, Q.y, Q.z, lo4, hi4) < cq)) {
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
            const lsk::Col<uint32_t, kFill> ids{A.perm};
            // (c.a: input row, c.b: the candidate's own cutoff)
            auto cand = [&](const auto &c, bool &use) {
              if ((!kPeriodic || c.mine) && c.d2 < rule<kBoth>(cq, c.b)) {
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
            };
            int cnt;
            if constexpr (kPeriodic)
              cnt = lsk::scan_bucket(T, node, lane, Q, ImageDiff{F, I}, ids, lsk::FloatCol{A.pcut2}, use, cand);
            else
              cnt = lsk::scan_bucket(T, node, lane, Q, lsk::OpenDiff{}, ids, lsk::FloatCol{A.pcut2}, use, cand);
            if (cnt) s_buckets++;
            if (evals) s_evals += (uint32_t)cnt;
          });
    };
    if constexpr (kPeriodic) {
      const Frame F = make_frame(T, A.L, gb);
      const float rmax = lsk::uniform_f(((const float4 *)T.nodes)[2].w);  // the largest cp of all
      const float thr = rule<kBoth>(gmax, rmax);
      for (int im = 0; im < 27; im++) {  // (wave-uniform)
        Image I;
        if (!image_of(F.X, F.Y, F.Z, im, I)) continue;
        if (!(image_box_dist2(gb, F.rlo, F.rhi, I) < thr)) continue;
        s_images++;
        cov.clear();
        walk(F, I);
      }
    } else {
      walk(Frame{}, Image{});
    }
  }

  if (!kFill) {
    if (Q.valid) A.counts[row] = (int32_t)count;
    lsk::add_stats<kPeriodic>(A.stats, lane, s_evals, s_nodes, s_buckets, s_accepts, lane == 0 ? s_images : 0u);
  } else if (Q.valid && (bad || cur != end)) {
    atomicAdd(A.err, 1u);
  }
}

// The arguments both entry points share. period: null for the open box, else three values > 0
// (+inf: open axis); the caller has checked every cutoff against it.
int reach_args(const char *what, const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *qcut2,
               const float *pcut2, int rule, const float *period, const uint32_t *out_perm, ReachArgs *A) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 32)) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)) "
                                            "or nq not in [0, 2^32)");
    return 1;
  }
  if (rule != LSK_REACH_EITHER && rule != LSK_REACH_BOTH) {
    lsk::set_last_error(std::string(what) + ": rule must be LSK_REACH_EITHER or LSK_REACH_BOTH");
    return 1;
  }
  *A = ReachArgs{};
  for (int a = 0; a < 3; a++) {
    const float v = period ? period[a] : __builtin_inff();
    if (!(v > 0.f)) {
      lsk::set_last_error(std::string(what) + ": period must be three values > 0 (+inf: open axis)");
      return 1;
    }
    A->L[a] = v;
  }
  if (!pcut2 || (nq > 0 && (!qpts || !out_perm || !qcut2))) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  A->T = *tree;
  A->qpts = qpts;
  A->nq = nq;
  A->qcut2 = qcut2;
  A->pcut2 = pcut2;
  A->out_perm = out_perm;
  return 0;
}

template <bool kFill>
void reach_launch(const ReachArgs &A, int rule, bool periodic, hipStream_t stream) {
  const unsigned blocks = lsk_blocks((A.nq + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  const bool both = rule == LSK_REACH_BOTH;
  if (both && periodic)
    radius_reach_walk_kernel<true, true, kFill><<<blocks, kWaves * 64, 0, stream>>>(A);
  else if (both)
    radius_reach_walk_kernel<true, false, kFill><<<blocks, kWaves * 64, 0, stream>>>(A);
  else if (periodic)
    radius_reach_walk_kernel<false, true, kFill><<<blocks, kWaves * 64, 0, stream>>>(A);
  else
    radius_reach_walk_kernel<false, false, kFill><<<blocks, kWaves * 64, 0, stream>>>(A);
}

}  // namespace

extern "C" int lsk_hip_radius_reach_count(const lsk_tree_view *tree, const float *qpts, int64_t nq,
                                          const float *qcut2, const float *pcut2, int rule, const float *period,
                                          const uint32_t *out_perm, int32_t *counts, unsigned long long *stats,
                                          void *stream) {
  ReachArgs A;
  if (reach_args("radius_reach_count", tree, qpts, nq, qcut2, pcut2, rule, period, out_perm, &A)) return 1;
  if (nq == 0) return 0;
  if (!counts) {
    lsk::set_last_error("radius_reach_count: null argument");
    return 1;
  }
  A.counts = counts;
  A.stats = stats;
  reach_launch<false>(A, rule, period != nullptr, (hipStream_t)stream);
  LSK_CHECK_LAUNCH("radius_reach_count");
  return 0;
}

extern "C" int lsk_hip_radius_reach_fill(const lsk_tree_view *tree, const uint32_t *perm, const float *qpts,
                                         int64_t nq, const float *qcut2, const float *pcut2, int rule,
                                         const float *period, const uint32_t *out_perm, const int64_t *offsets,
                                         int32_t *out_idx, float *out_dist, uint32_t *err, void *stream) {
  ReachArgs A;
  if (reach_args("radius_reach_fill", tree, qpts, nq, qcut2, pcut2, rule, period, out_perm, &A)) return 1;
  if (nq == 0) return 0;
  // (out_idx / out_dist may be null when every row is empty, as in lsk_hip_radius_fill)
  if (!perm || !offsets || !err) {
    lsk::set_last_error("radius_reach_fill: null argument");
    return 1;
  }
  A.perm = perm;
  A.offsets = offsets;
  A.out_idx = out_idx;
  A.out_dist = (uint32_t *)out_dist;
  A.err = err;
  reach_launch<true>(A, rule, period != nullptr, (hipStream_t)stream);
  LSK_CHECK_LAUNCH("radius_reach_fill");
  return 0;
}
