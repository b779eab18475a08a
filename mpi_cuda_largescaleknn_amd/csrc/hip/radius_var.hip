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

// scan_bucket of ball_walk.h with the candidates' own cut2 travelling beside them:
// cand(d2, cut2 of the point, id, use).
template <bool kIds, class Cand>
__device__ __forceinline__ int scan_bucket_cut(const lsk_tree_view &T, const uint32_t *perm, const float *pcut2,
                                               uint32_t node, int lane, const lsk::GroupQuery &Q, bool &use,
                                               Cand cand) {
  const int64_t base = ((int64_t)node - ((int64_t)1 << T.depth)) * lsk::kBucket;
  if (base >= T.n) return 0;
  const int cnt = (int)min((int64_t)lsk::kBucket, T.n - base);
  const int64_t pi = base + lane;
  float px = 0.f, py = 0.f, pz = 0.f, pc = 0.f;
  uint32_t pid = 0;
  if (lane < cnt) {
    px = T.pts[3 * pi];
    py = T.pts[3 * pi + 1];
    pz = T.pts[3 * pi + 2];
    pc = pcut2[pi];
    if (kIds) pid = perm[pi];
  }
  for (int j = 0; j < cnt; j++) {
    const float x = lsk::readlane_f(px, j), y = lsk::readlane_f(py, j), z = lsk::readlane_f(pz, j);
    const float c = lsk::readlane_f(pc, j);
    uint32_t id = 0;
    if (kIds) id = (uint32_t)__builtin_amdgcn_readlane((int)pid, j);
    if (use) cand(lsk::dist2(Q.x - x, Q.y - y, Q.z - z), c, id, use);
  }
  return cnt;
}

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
  // gather count: as radius.hip, the lane took a whole node when the stack stood at cov_sp
  bool cov = false;
  uint32_t cov_sp = 0;
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
            if (cov && sp < cov_sp) cov = false;
            use = use && !cov;
            if (use) {
              const float fx = fmaxf(fabsf(lo4.x - qx), fabsf(hi4.x - qx));
              const float fy = fmaxf(fabsf(lo4.y - qy), fabsf(hi4.y - qy));
              const float fz = fmaxf(fabsf(lo4.z - qz), fabsf(hi4.z - qz));
              if (lsk::dist2(fx, fy, fz) < cut2) {
                // the node's points: its buckets, the last one clipped at n
                const int32_t span_lg = T.depth - lvl;
                const int64_t first = ((int64_t)node - ((int64_t)1 << lvl)) << span_lg;
                const int64_t p0 = first * lsk::kBucket;
                const int64_t p1 = min(T.n, (first + ((int64_t)1 << span_lg)) * lsk::kBucket);
                if (p1 > p0) count += (uint32_t)(p1 - p0);
                cov = true;
                cov_sp = sp;
                use = false;
                s_accepts++;
              }
            }
          }
          return use;
        },
        [&](uint32_t node, bool use) {
          const bool evals = use;
          int cnt;
          if (kScatter) {
            cnt = scan_bucket_cut<kFill>(T, A.perm, A.pcut2, node, lane, Q, use, take);
          } else {
            cnt = lsk::scan_bucket<kFill>(T, A.perm, node, lane, Q, use,
                                          [&](float d2, uint32_t id, bool &use) { take(d2, cut2, id, use); });
          }
          if (cnt) s_buckets++;
          if (evals) s_evals += (uint32_t)cnt;
        });
  }

  if (!kFill) {
    if (Q.valid) A.counts[row] = (int32_t)count;
    if (A.stats) {
      const uint32_t e = lsk::wave_sum(s_evals), a = lsk::wave_sum(s_accepts);
      if (lane == 0) {
        atomicAdd(&A.stats[0], (unsigned long long)e);
        atomicAdd(&A.stats[1], (unsigned long long)s_nodes);
        atomicAdd(&A.stats[2], (unsigned long long)s_buckets);
        atomicAdd(&A.stats[3], (unsigned long long)a);
      }
    }
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
