// Variable-radius search: the count and fill walks of radius.hip with a squared cutoff per
// query (gather: p is in row q iff d² < cut2[q]) or per indexed point (scatter: iff d² <
// cut2[p]). Rows, offsets, the error word and the statistics are those of radius.hip; the
// rows are sorted and finalised by lsk_hip_radius_sort unchanged.
//
//  gather   a lane reads its own cut2 at its query row. A lane is live iff its query is
//           finite and its cut2 > 0; the group cull uses the largest cut2 of the live lanes,
//           the per-lane node test, the far-corner acceptance and the candidate test the
//           lane's own. A group therefore descends as deep as its widest lane needs; lanes
//           with a smaller radius drop out node by node.
//  scatter  the walk runs over a copy of the node array whose lo.w holds the largest cut2 of
//           the points below each node (lsk_hip_tree_set_radii over the curve-ordered cut2).
//           A node is culled against the group, and tested per lane, with its own lo.w. No
//           far-corner acceptance: it would need the smallest cut2 below a node, which the
//           tree does not store. A candidate's cut2 is loaded one per lane with the bucket's
//           points and broadcast beside the coordinates.
#include "ball_walk.h"

namespace {

using lsk::fbits;

constexpr int kWaves = 4;  // waves per block, one query group each (as radius.hip)

struct RadVarArgs {
  lsk_tree_view T;           // scatter: T.nodes is the annotated copy
  const uint32_t *perm;      // sorted position -> input row (fill)
  const float *qpts;         // sorted queries
  int64_t nq;
  const float *qcut2;        // gather: [nq], query order
  const float *pcut2;        // scatter: [n], curve order
  const uint32_t *out_perm;  // sorted query -> query row
  int32_t *counts;           // count: [nq], query order
  const int64_t *offsets;    // fill: [nq + 1], query order
  int32_t *out_idx;          // fill: [total]
  uint32_t *out_dist;        // fill: [total] d² bits until lsk_hip_radius_sort finalises them
  uint32_t *err;             // fill
  unsigned long long *stats; // count, optional [4], as radius.hip
};

template <bool kScatter, bool kFill>
__global__ __launch_bounds__(kWaves * 64) void radius_var_walk_kernel(const RadVarArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= A.nq) return;  // (wave-uniform)
  const lsk::GroupQuery Q = lsk::load_group(g, lane, A.qpts, A.out_perm, A.nq);
  const float qx = Q.x, qy = Q.y, qz = Q.z;
  const int64_t row = Q.row;
  // gather: the lane's own cutoff; scatter: unused (every cutoff comes from the tree's side)
  float cut2 = 0.f;
  if (!kScatter && Q.valid) cut2 = A.qcut2[row];
  int64_t cur = 0, end = 0;
  if (kFill && Q.valid) {
    cur = A.offsets[row];
    end = A.offsets[row + 1];
  }
  const bool live = Q.finite && (kScatter || cut2 > 0.f);
  uint32_t count = 0;
  bool bad = false;
  lsk::Cover cov;  // gather count: the whole node the lane took
  uint32_t s_evals = 0, s_accepts = 0, s_nodes = 0, s_buckets = 0;

  if (__ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    const float gmax = kScatter ? 0.f : lsk::wave_max(live ? cut2 : 0.f);
    const lsk::vec3f q{qx, qy, qz};
    const lsk_tree_view &T = A.T;
    auto take = [&](float d2, float c, uint32_t id, bool &use) {
      if (d2 < c) {
        if (!kFill) {
          count++;
        } else if (cur < end) {
          A.out_idx[cur] = (int32_t)id;
          A.out_dist[cur] = fbits(d2);
          cur++;
        } else {  // more than the count pass saw: stop appending
          bad = true;
          use = false;
        }
      }
    };
    lsk::ball_walk<true>(
        T, stk_all[wid], lane,
        [&](const float4 &lo4, const float4 &hi4) {
          return lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4)) < (kScatter ? lo4.w : gmax);
        },
        [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
          s_nodes++;
          const float c = kScatter ? lo4.w : cut2;
          bool use = live && !bad && lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}) < c;
          if (!kScatter && !kFill) {
            cov.pop(sp);
            use = use && !cov.on();
            if (use && lsk::far_dist2(qx, qy, qz, lo4, hi4) < cut2) {
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
          int cnt;
          if (kScatter) {  // the candidate's own cutoff travels beside it
            cnt = lsk::scan_bucket(T, node, lane, Q, lsk::OpenDiff{}, ids, lsk::FloatCol{A.pcut2}, use,
                                   [&](const auto &c, bool &use) { take(c.d2, c.b, c.a, use); });
          } else {
            cnt = lsk::scan_bucket(T, node, lane, Q, lsk::OpenDiff{}, ids, lsk::NoCol{}, use,
                                   [&](const auto &c, bool &use) { take(c.d2, cut2, c.a, use); });
          }
          if (cnt) s_buckets++;
          if (evals) s_evals += (uint32_t)cnt;
        });
  }

  if (!kFill) {
    if (Q.valid) A.counts[row] = (int32_t)count;
    lsk::add_stats<false>(A.stats, lane, s_evals, s_nodes, s_buckets, s_accepts);
  } else if (Q.valid && (bad || cur != end)) {
    atomicAdd(A.err, 1u);
  }
}

// The arguments both entry points share; exactly one of qcut2 / pcut2 is given.
int var_args(const char *what, const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *qcut2,
             const float *pcut2, const uint32_t *out_perm, RadVarArgs *A) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 32)) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)) "
                                            "or nq not in [0, 2^32)");
    return 1;
  }
  if ((qcut2 != nullptr) == (pcut2 != nullptr)) {
    lsk::set_last_error(std::string(what) + ": exactly one of qcut2 (per query) and pcut2 (per point) is given");
    return 1;
  }
  if (nq > 0 && (!qpts || !out_perm)) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  *A = RadVarArgs{};
  A->T = *tree;
  A->qpts = qpts;
  A->nq = nq;
  A->qcut2 = qcut2;
  A->pcut2 = pcut2;
  A->out_perm = out_perm;
  return 0;
}

}  // namespace

extern "C" int lsk_hip_radius_var_count(const lsk_tree_view *tree, const float *qpts, int64_t nq,
                                        const float *qcut2, const float *pcut2, const uint32_t *out_perm,
                                        int32_t *counts, unsigned long long *stats, void *stream) {
  RadVarArgs A;
  if (var_args("radius_var_count", tree, qpts, nq, qcut2, pcut2, out_perm, &A)) return 1;
  if (nq == 0) return 0;
  if (!counts) {
    lsk::set_last_error("radius_var_count: null argument");
    return 1;
  }
  A.counts = counts;
  A.stats = stats;
  const unsigned blocks = lsk_blocks((nq + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  if (pcut2)
    radius_var_walk_kernel<true, false><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  else
    radius_var_walk_kernel<false, false><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("radius_var_count");
  return 0;
}

extern "C" int lsk_hip_radius_var_fill(const lsk_tree_view *tree, const uint32_t *perm, const float *qpts,
                                       int64_t nq, const float *qcut2, const float *pcut2,
                                       const uint32_t *out_perm, const int64_t *offsets, int32_t *out_idx,
                                       float *out_dist, uint32_t *err, void *stream) {
  RadVarArgs A;
  if (var_args("radius_var_fill", tree, qpts, nq, qcut2, pcut2, out_perm, &A)) return 1;
  if (nq == 0) return 0;
  // (out_idx / out_dist may be null when every row is empty, as in lsk_hip_radius_fill)
  if (!perm || !offsets || !err) {
    lsk::set_last_error("radius_var_fill: null argument");
    return 1;
  }
  A.perm = perm;
  A.offsets = offsets;
  A.out_idx = out_idx;
  A.out_dist = (uint32_t *)out_dist;
  A.err = err;
  const unsigned blocks = lsk_blocks((nq + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  if (pcut2)
    radius_var_walk_kernel<true, true><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  else
    radius_var_walk_kernel<false, true><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("radius_var_fill");
  return 0;
}
