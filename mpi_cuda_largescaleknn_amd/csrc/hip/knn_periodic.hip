// Periodic k-NN: the k-th distance and the neighbour lists of foreign queries under a period
// (the contract of periodic.hip, without its radius bound), from the open-box results.
//
// Exactness. pd2(q, p) <= d2(q, p) for every pair, in float32: a wrap replaces a difference d
// > h = 0.5f L by fl(d - L), and -d < d - L < d because 2 d > L, so the exact value is smaller
// in magnitude than the float d and rounding to nearest cannot pass d; the mirrored branch
// alike; products and fmaf are monotone in the magnitudes. The open-box k-th squared distance
// b of a query (the cutoff where fewer than k points qualify) therefore bounds its periodic
// one, and every point of the periodic answer has pd2 <= b, i.e. pd2 < cutq with cutq = the
// float after b, or cut2 itself when b is the cutoff.
//
// Flag. A query is flagged iff for some image s != 0 that its group can take the slackened
// gap between the query moved by s and the root box is below cutq. A point p with wrap vector
// w(q, p) = s != 0 and pd2 < cutq makes the group take s (make_axis: monotone differences)
// and has gap <= pd2 (the cull proof of periodic.hip, which argues per pair and never uses
// the radius bound), so an unflagged query has only points of wrap vector 0 below cutq: for
// them pd2 == d2 bit for bit, the sets { pd2 < cutq } and { d2 < cutq } coincide, and the
// open-box k-th value and list are the periodic ones.
//
// Flagged queries run a periodic radius search with their own cutoff cutq over the compacted
// list (the image loop, cull and candidate test of periodic.hip's walks: a pair counts in the
// one image that is its wrap vector; every pair has one in {-1, 0, +1}^3, so the 27 images are
// complete for any cutq). The count walk has no whole-box acceptance: the rows are a few
// times k long and the walk is short. Rows are sorted by lsk_hip_radius_sort; the take kernel
// writes the first k of each.
#include "periodic_image.h"

namespace {

using lsk::fbits;
using namespace lsk::periodic;

constexpr int kWaves = 4;  // waves per block, one group of 64 queries each

struct PknnFlagArgs {
  lsk_tree_view T;
  const float *qpts;  // sorted queries
  const float *d2;    // [nq] open-box k-th d², sorted order
  int64_t nq;
  float cut2;
  float L[3];
  float *cutq;        // [nq] sorted order
  int32_t *flags;     // [nq] sorted order
};

__global__ __launch_bounds__(kWaves * 64) void pknn_flag_kernel(const PknnFlagArgs A) {
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= A.nq) return;  // (wave-uniform)
  lsk::GroupQuery Q{g * lsk::kBucket + lane, 0, 0.f, 0.f, 0.f, false, false};
  Q.valid = Q.qi < A.nq;
  float cutq = A.cut2;
  if (Q.valid) {
    Q.x = A.qpts[3 * Q.qi];
    Q.y = A.qpts[3 * Q.qi + 1];
    Q.z = A.qpts[3 * Q.qi + 2];
    const float b = A.d2[Q.qi];
    if (b < A.cut2) cutq = lsk::bitsf(fbits(b) + 1u);  // the closed bound as a strict cutoff
  }
  Q.finite = Q.valid && lsk::finite3(Q.x, Q.y, Q.z);
  const bool live = Q.finite && cutq > 0.f;
  bool flag = false;
  if (__ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    const Frame F = make_frame(A.T, A.L, gb);
    for (int im = 0; im < 27; im++) {  // (wave-uniform)
      Image I;
      if (im == 13 || !image_of(F.X, F.Y, F.Z, im, I)) continue;
      if (live && image_point_dist2(Q, F.rlo, F.rhi, I) < cutq) flag = true;
    }
  }
  if (Q.valid) {
    A.cutq[Q.qi] = cutq;
    A.flags[Q.qi] = flag ? 1 : 0;
  }
}

struct PknnWalkArgs {
  lsk_tree_view T;
  const uint32_t *perm;      // sorted position -> input row (fill)
  const float *qpts;         // sorted queries
  const int32_t *list;       // [m] flagged sorted queries, ascending
  int64_t m;
  const float *cutq;         // [nq] sorted order
  float L[3];
  int32_t *counts;           // count: [m], list order
  const int64_t *offsets;    // fill: [m + 1], list order
  int32_t *out_idx;          // fill: [total]
  uint32_t *out_dist;        // fill: [total] pd2 bits until lsk_hip_radius_sort finalises them
  uint32_t *err;             // fill
  unsigned long long *stats; // count, optional [5]: evaluations, nodes, buckets, 0, image walks
};

// radius_periodic_walk_kernel<true, *> of periodic.hip driven by the list: lane's query =
// qpts[list[g 64 + lane]], its cutoff cutq of that query, its row the list entry.
template <bool kFill>
__global__ __launch_bounds__(kWaves * 64) void pknn_walk_kernel(const PknnWalkArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= A.m) return;  // (wave-uniform)
  const int64_t row = g * lsk::kBucket + lane;
  lsk::GroupQuery Q{0, row, 0.f, 0.f, 0.f, false, false};
  Q.valid = row < A.m;
  float cut2 = 0.f;
  int64_t cur = 0, end = 0;
  if (Q.valid) {
    Q.qi = (int64_t)A.list[row];
    Q.x = A.qpts[3 * Q.qi];
    Q.y = A.qpts[3 * Q.qi + 1];
    Q.z = A.qpts[3 * Q.qi + 2];
    cut2 = A.cutq[Q.qi];
    if (kFill) {
      cur = A.offsets[row];
      end = A.offsets[row + 1];
    }
  }
  Q.finite = Q.valid && lsk::finite3(Q.x, Q.y, Q.z);
  const bool live = Q.finite && cut2 > 0.f;
  uint32_t count = 0;
  bool bad = false;
  uint32_t s_evals = 0, s_nodes = 0, s_buckets = 0, s_images = 0;

  if (__ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    const float gmax = lsk::wave_max(live ? cut2 : 0.f);
    const lsk_tree_view &T = A.T;
    const Frame F = make_frame(T, A.L, gb);
    for (int im = 0; im < 27; im++) {  // (wave-uniform)
      Image I;
      if (!image_of(F.X, F.Y, F.Z, im, I)) continue;
      if (!(image_box_dist2(gb, F.rlo, F.rhi, I) < gmax)) continue;
      s_images++;
      lsk::ball_walk<true>(
          T, stk_all[wid], lane,
          [&](const float4 &lo4, const float4 &hi4) { return image_box_dist2(gb, lo4, hi4, I) < gmax; },
          [&](uint32_t, int32_t, uint32_t, const float4 &lo4, const float4 &hi4) {
            s_nodes++;
            return live && !bad && image_point_dist2(Q, lo4, hi4, I) < cut2;
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
    lsk::add_stats<true>(A.stats, lane, s_evals, s_nodes, s_buckets, 0u, lane == 0 ? s_images : 0u);
  } else if (Q.valid && (bad || cur != end)) {
    atomicAdd(A.err, 1u);
  }
}

struct PknnTakeArgs {
  const int32_t *list;      // [m] flagged sorted queries
  int64_t m;
  const int64_t *offsets;   // [m + 1] the sorted rows (idx, final distances)
  const int32_t *idx;
  const float *dist;
  const uint32_t *qperm;    // sorted query -> query row
  const float *d2;          // [nq] open-box k-th d², sorted order
  float cut2;
  int32_t k;
  float *out;               // [nq] query order
  int32_t *out_idx;         // [nq][k] or null
  float *out_dist;          // [nq][k] or null
  uint32_t *err;
};

// Element t: slot j = t % k of list entry e = t / k (lists), or slot k - 1 of entry t.
__global__ __launch_bounds__(256) void pknn_take_kernel(const PknnTakeArgs A) {
  const bool lists = A.out_idx != nullptr;
  const int64_t total = lists ? A.m * (int64_t)A.k : A.m;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const int64_t e = lists ? t / A.k : t;
    const int32_t j = lists ? (int32_t)(t - e * A.k) : A.k - 1;
    const int64_t qi = (int64_t)A.list[e];
    const int64_t row = (int64_t)A.qperm[qi];
    const int64_t o = A.offsets[e], len = A.offsets[e + 1] - o;
    const bool have = (int64_t)j < len;
    const float d = have ? A.dist[o + j] : lsk::final_distance(A.cut2);
    if (lists) {
      A.out_idx[row * A.k + j] = have ? A.idx[o + j] : -1;
      A.out_dist[row * A.k + j] = d;
    }
    if (j == A.k - 1) {
      A.out[row] = d;
      // fewer than k although the open-box pass found k below the cutoff: the bound was none
      if (!have && A.d2[qi] < A.cut2) atomicAdd(A.err, 1u);
    }
  }
}

int pknn_period(const char *what, const float *period, float *L) {
  for (int a = 0; a < 3; a++) {
    const float v = period ? period[a] : 0.f;
    if (!(v > 0.f)) {
      lsk::set_last_error(std::string(what) + ": period must be three values > 0 (+inf: open axis)");
      return 1;
    }
    L[a] = v;
  }
  return 0;
}

int pknn_walk_args(const char *what, const lsk_tree_view *tree, const float *qpts, const int32_t *list, int64_t m,
                   const float *cutq, const float *period, PknnWalkArgs *A) {
  if (!lsk_tree_ok(tree) || m < 0 || m >= ((int64_t)1 << 31)) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)) "
                                            "or not 0 <= m < 2^31");
    return 1;
  }
  *A = PknnWalkArgs{};
  if (pknn_period(what, period, A->L)) return 1;
  if (m > 0 && (!qpts || !list || !cutq)) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  A->T = *tree;
  A->qpts = qpts;
  A->list = list;
  A->m = m;
  A->cutq = cutq;
  return 0;
}

}  // namespace

extern "C" int lsk_hip_pknn_flag(const lsk_tree_view *tree, const float *qpts, const float *d2, int64_t nq,
                                 float cut2, const float *period, float *cutq, int32_t *flags, void *stream) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 31) || !(cut2 >= 0.f)) {
    lsk::set_last_error("pknn_flag: tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)), "
                        "0 <= nq < 2^31 or cut2 not >= 0");
    return 1;
  }
  PknnFlagArgs A{};
  if (pknn_period("pknn_flag", period, A.L)) return 1;
  if (nq == 0) return 0;
  if (!qpts || !d2 || !cutq || !flags) {
    lsk::set_last_error("pknn_flag: null argument");
    return 1;
  }
  A.T = *tree;
  A.qpts = qpts;
  A.d2 = d2;
  A.nq = nq;
  A.cut2 = cut2;
  A.cutq = cutq;
  A.flags = flags;
  const unsigned blocks = lsk_blocks((nq + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  pknn_flag_kernel<<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("pknn_flag");
  return 0;
}

extern "C" int lsk_hip_pknn_count(const lsk_tree_view *tree, const float *qpts, const int32_t *list, int64_t m,
                                  const float *cutq, const float *period, int32_t *counts,
                                  unsigned long long *stats, void *stream) {
  PknnWalkArgs A;
  if (pknn_walk_args("pknn_count", tree, qpts, list, m, cutq, period, &A)) return 1;
  if (m == 0) return 0;
  if (!counts) {
    lsk::set_last_error("pknn_count: null argument");
    return 1;
  }
  A.counts = counts;
  A.stats = stats;
  const unsigned blocks = lsk_blocks((m + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  pknn_walk_kernel<false><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("pknn_count");
  return 0;
}

extern "C" int lsk_hip_pknn_fill(const lsk_tree_view *tree, const uint32_t *perm, const float *qpts,
                                 const int32_t *list, int64_t m, const float *cutq, const float *period,
                                 const int64_t *offsets, int32_t *out_idx, float *out_dist, uint32_t *err,
                                 void *stream) {
  PknnWalkArgs A;
  if (pknn_walk_args("pknn_fill", tree, qpts, list, m, cutq, period, &A)) return 1;
  if (m == 0) return 0;
  // (out_idx / out_dist may be null when every row is empty, as in lsk_hip_radius_fill)
  if (!perm || !offsets || !err) {
    lsk::set_last_error("pknn_fill: null argument");
    return 1;
  }
  A.perm = perm;
  A.offsets = offsets;
  A.out_idx = out_idx;
  A.out_dist = (uint32_t *)out_dist;
  A.err = err;
  const unsigned blocks = lsk_blocks((m + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  pknn_walk_kernel<true><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("pknn_fill");
  return 0;
}

extern "C" int lsk_hip_pknn_take(const int32_t *list, int64_t m, const int64_t *offsets, const int32_t *idx,
                                 const float *dist, const uint32_t *qperm, const float *d2, float cut2, int32_t k,
                                 float *out, int32_t *out_idx, float *out_dist, uint32_t *err, void *stream) {
  if (m < 0 || m >= ((int64_t)1 << 31) || k < 1 || !(cut2 >= 0.f) || (out_idx == nullptr) != (out_dist == nullptr)) {
    lsk::set_last_error("pknn_take: not 0 <= m < 2^31, k < 1, cut2 not >= 0 or one of out_idx / out_dist alone");
    return 1;
  }
  if (m == 0) return 0;
  // (idx / dist may be null when every row is empty: no slot of such a row is read)
  if (!list || !offsets || !qperm || !d2 || !out || !err) {
    lsk::set_last_error("pknn_take: null argument");
    return 1;
  }
  PknnTakeArgs A{list, m, offsets, idx, dist, qperm, d2, cut2, k, out, out_idx, out_dist, err};
  const int64_t threads = out_idx ? m * (int64_t)k : m;
  pknn_take_kernel<<<lsk_blocks(threads, 256, 1u << 20), 256, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("pknn_take");
  return 0;
}
