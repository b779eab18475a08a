// Fixed-radius search: for every query the number of points with d² < cut2, and those
// points themselves as CSR rows (ids in input order + distances).
//
// No selection pass: a radius query is the group walk of ball_walk.h with the same radius
// in every lane, run twice (count, then fill into rows sized by the counts), plus a sort
// over rows of varying length.
//
//  1. radius_walk_kernel<false> (count): a box is pruned when it is not closer than cut2 to
//     the group's box. Every popped node is tested per lane: nearer corner >= cut2: nothing of
//     it counts for the lane; farthest corner < cut2: all of it does, so the lane adds the
//     node's population (clipped at n) without a distance evaluation and ignores the node's
//     subtree. Per-axis float differences, squares and fma are monotone, so no point inside
//     a box has a larger computed d² than its farthest corner (knn_exact.hip::count_tree
//     carries the same argument): the shortcut is exact for finite points. The subtree is
//     descended only for the lanes that are neither; its points are tested one by one.
//  2. radius_walk_kernel<true> (fill): the same walk and pruning without the shortcut (a
//     row needs every d² anyway). A lane appends (d² bits, perm[pos]) into its own row
//     [offsets[row], offsets[row + 1]) and never writes past the row's end; a lane that
//     would, or that ends short of it, bumps the error word (count and fill disagree: a bug).
//  3. radius_sort_lds_kernel: rows of up to kLdsRow pairs, sorted in place by
//     (d² bits << 32 | id) with the LDS network of row_sort.h, 32 consecutive rows per block
//     padded to the longest of them, then final_distance. radius_sort_big_kernel: longer
//     rows, one block per row, the same keys by an all-ascending bitonic network over
//     global memory (any length: the virtual padding up to the next power of two is +inf
//     and never moves, so comparators that reach past the row's end are skipped).
#include "ball_walk.h"
#include "row_sort.h"

namespace {

using lsk::fbits;
using lsk::finalised;

constexpr int kWaves = 4;      // waves per block, one query group each
// Longest row the LDS sort takes: 4096 64-bit keys = 32 KB per block, so four blocks (and
// their 16 waves) share a CU's 160 KB; twice that would halve the blocks of the common
// short-row case for rows that are rare.
constexpr int kLdsRow = 4096;
constexpr int kSortRows = 32;  // consecutive rows per LDS sort block
constexpr int kSortThreads = 256;
constexpr int kBigThreads = 1024;

struct RadArgs {
  lsk_tree_view T;
  const uint32_t *perm;      // sorted position -> input row (fill)
  const float *qpts;         // sorted queries
  int64_t nq;
  float cut2;
  const uint32_t *out_perm;  // sorted query -> query row
  int32_t *counts;           // count: [nq], query order
  const int64_t *offsets;    // fill: [nq + 1], query order
  int32_t *out_idx;          // fill: [total]
  uint32_t *out_dist;        // fill: [total] d² bits until the sort kernels finalise them
  uint32_t *err;             // fill
  unsigned long long *stats; // count, optional [4]: distance evaluations, nodes popped,
                             // buckets scanned, whole-box acceptances
};

template <bool kFill>
__global__ __launch_bounds__(kWaves * 64) void radius_walk_kernel(const RadArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= A.nq) return;  // (wave-uniform)
  const lsk::GroupQuery Q = lsk::load_group(g, lane, A.qpts, A.out_perm, A.nq);
  const float cut2 = A.cut2;
  const float qx = Q.x, qy = Q.y, qz = Q.z;
  const int64_t row = Q.row;
  int64_t cur = 0, end = 0;
  if (kFill && Q.valid) {
    cur = A.offsets[row];
    end = A.offsets[row + 1];
  }
  const bool live = Q.finite && cut2 > 0.f;
  uint32_t count = 0;
  bool bad = false;
  lsk::Cover cov;  // count: the whole node the lane took
  uint32_t s_evals = 0, s_accepts = 0, s_nodes = 0, s_buckets = 0;

  if (__ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    const lsk::vec3f q{qx, qy, qz};
    const lsk_tree_view &T = A.T;
    lsk::ball_walk<true>(
        T, stk_all[wid], lane,
        [&](const float4 &lo4, const float4 &hi4) { return lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4)) < cut2; },
        [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
          s_nodes++;
          bool use = live && !bad && lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}) < cut2;
          if (!kFill) {
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
        // a bucket: the lanes that need it test its points one by one
        [&](uint32_t node, bool use) {
          const bool evals = use;
          const int cnt = lsk::scan_bucket(T, node, lane, Q, lsk::OpenDiff{}, lsk::Col<uint32_t, kFill>{A.perm},
                                           lsk::NoCol{}, use, [&](const auto &c, bool &use) {
            if (c.d2 < cut2) {
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

  if (!kFill) {
    if (Q.valid) A.counts[row] = (int32_t)count;
    lsk::add_stats<false>(A.stats, lane, s_evals, s_nodes, s_buckets, s_accepts);
  } else if (Q.valid && (bad || cur != end)) {
    atomicAdd(A.err, 1u);
  }
}

// Rows [blockIdx * kSortRows, + kSortRows) that fit the LDS, kLdsRow >> lg at a time, each
// padded to 2^lg keys, 2^lg >= the longest of them.
__global__ __launch_bounds__(kSortThreads) void radius_sort_lds_kernel(const int64_t *__restrict__ offsets,
                                                                       int32_t *__restrict__ idx,
                                                                       uint32_t *__restrict__ dist, int64_t nq) {
  __shared__ uint64_t key[kLdsRow];
  __shared__ int64_t off[kSortRows + 1];
  __shared__ uint32_t longest;
  const int64_t row0 = (int64_t)blockIdx.x * kSortRows;
  const uint32_t nrows = (uint32_t)min((int64_t)kSortRows, nq - row0);
  if (threadIdx.x == 0) longest = 0u;
  if (threadIdx.x <= nrows) off[threadIdx.x] = offsets[row0 + threadIdx.x];
  __syncthreads();
  if (threadIdx.x < nrows) {
    const int64_t len = off[threadIdx.x + 1] - off[threadIdx.x];
    if (len > 0 && len <= (int64_t)kLdsRow) atomicMax(&longest, (uint32_t)len);
  }
  __syncthreads();
  const uint32_t m = longest;
  if (m == 0u) return;  // (block-uniform: nothing but empty rows and rows of the other kernel)
  const uint32_t lg = m <= 1u ? 0u : 32u - (uint32_t)__clz(m - 1u);
  const uint32_t kpad = 1u << lg;
  const uint32_t rows_per_pass = (uint32_t)kLdsRow >> lg;
  for (uint32_t r0 = 0; r0 < nrows; r0 += rows_per_pass) {
    for (uint32_t e = threadIdx.x; e < (uint32_t)kLdsRow; e += kSortThreads) {
      const uint32_t r = r0 + (e >> lg), c = e & (kpad - 1u);
      uint64_t v = ~0ull;
      if (r < nrows) {
        const int64_t len = off[r + 1] - off[r];
        if (len <= (int64_t)kLdsRow && (int64_t)c < len) {
          const int64_t o = off[r] + c;
          v = lsk::pack_key(dist[o], idx[o]);
        }
      }
      key[e] = v;
    }
    __syncthreads();
    lsk::sort_rows_lds(key, kLdsRow, kpad, kSortThreads);
    for (uint32_t e = threadIdx.x; e < (uint32_t)kLdsRow; e += kSortThreads) {
      const uint32_t r = r0 + (e >> lg), c = e & (kpad - 1u);
      if (r < nrows) {
        const int64_t len = off[r + 1] - off[r];
        if (len <= (int64_t)kLdsRow && (int64_t)c < len) {
          const int64_t o = off[r] + c;
          const uint64_t v = key[e];
          idx[o] = lsk::key_id(v);
          dist[o] = finalised(lsk::key_d2bits(v));
        }
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void order_pair(int32_t *idx, uint32_t *dist, int64_t i, int64_t p) {
  const uint64_t a = lsk::pack_key(dist[i], idx[i]), b = lsk::pack_key(dist[p], idx[p]);
  if (a > b) {
    idx[i] = lsk::key_id(b);
    dist[i] = lsk::key_d2bits(b);
    idx[p] = lsk::key_id(a);
    dist[p] = lsk::key_d2bits(a);
  }
}

// Rows longer than kLdsRow, one block per row (blocks stride over all rows and skip the
// others). Every comparator of this form of the network orders its pair ascending (the
// first step of a merge mirrors the upper half instead of reversing the direction), so the
// virtual +inf keys at [len, 2^lg) never move and a comparator whose upper end is one of
// them is a no-op. A step's pairs are disjoint; __syncthreads orders the steps.
__global__ __launch_bounds__(kBigThreads) void radius_sort_big_kernel(const int64_t *__restrict__ offsets,
                                                                      int32_t *__restrict__ idx_all,
                                                                      uint32_t *__restrict__ dist_all, int64_t nq) {
  for (int64_t row = blockIdx.x; row < nq; row += gridDim.x) {
    const int64_t o0 = offsets[row];
    const int64_t len = offsets[row + 1] - o0;
    if (len <= (int64_t)kLdsRow) continue;  // (block-uniform)
    int32_t *idx = idx_all + o0;
    uint32_t *dist = dist_all + o0;
    int64_t P = (int64_t)kLdsRow * 2;
    while (P < len) P <<= 1;
    const int64_t half = P >> 1;
    int lgk = 1;
    for (int64_t kk = 2; kk <= P; kk <<= 1, lgk++) {
      const int64_t h = kk >> 1;
      for (int64_t t = threadIdx.x; t < half; t += kBigThreads) {
        const int64_t blk = (t >> (lgk - 1)) << lgk, o = t & (h - 1);
        const int64_t i = blk + o, p = blk + kk - 1 - o;
        if (p < len) order_pair(idx, dist, i, p);
      }
      __syncthreads();
      for (int64_t j = kk >> 2; j > 0; j >>= 1) {
        for (int64_t t = threadIdx.x; t < half; t += kBigThreads) {
          const int64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int64_t p = i | j;
          if (p < len) order_pair(idx, dist, i, p);
        }
        __syncthreads();
      }
    }
    for (int64_t t = threadIdx.x; t < len; t += kBigThreads) dist[t] = finalised(dist[t]);
  }
}

__global__ __launch_bounds__(256) void radius_finalise_kernel(uint32_t *__restrict__ dist, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
    dist[i] = finalised(dist[i]);
}

}  // namespace

extern "C" int lsk_hip_radius_lds_row(void) { return kLdsRow; }

extern "C" int lsk_hip_radius_count(const lsk_tree_view *tree, const float *qpts, int64_t nq, float cut2,
                                    const uint32_t *out_perm, int32_t *counts, unsigned long long *stats,
                                    void *stream) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 32) || !(cut2 >= 0.f)) {
    lsk::set_last_error("radius_count: tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)), "
                        "0 <= nq < 2^32 or cut2 not >= 0");
    return 1;
  }
  if (nq == 0) return 0;
  if (!qpts || !out_perm || !counts) {
    lsk::set_last_error("radius_count: null argument");
    return 1;
  }
  RadArgs A{};
  A.T = *tree;
  A.qpts = qpts;
  A.nq = nq;
  A.cut2 = cut2;
  A.out_perm = out_perm;
  A.counts = counts;
  A.stats = stats;
  const int64_t ngroups = (nq + lsk::kBucket - 1) / lsk::kBucket;
  radius_walk_kernel<false><<<lsk_blocks(ngroups, kWaves), kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("radius_count");
  return 0;
}

extern "C" int lsk_hip_radius_fill(const lsk_tree_view *tree, const uint32_t *perm, const float *qpts, int64_t nq,
                                   float cut2, const uint32_t *out_perm, const int64_t *offsets, int32_t *out_idx,
                                   float *out_dist, uint32_t *err, void *stream) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 32) || !(cut2 >= 0.f)) {
    lsk::set_last_error("radius_fill: tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)), "
                        "0 <= nq < 2^32 or cut2 not >= 0");
    return 1;
  }
  if (nq == 0) return 0;
  // (out_idx / out_dist may be null when every row is empty: nothing is written then, and a
  // lane that finds a point all the same bumps the error word before it stores)
  if (!perm || !qpts || !out_perm || !offsets || !err) {
    lsk::set_last_error("radius_fill: null argument");
    return 1;
  }
  RadArgs A{};
  A.T = *tree;
  A.perm = perm;
  A.qpts = qpts;
  A.nq = nq;
  A.cut2 = cut2;
  A.out_perm = out_perm;
  A.offsets = offsets;
  A.out_idx = out_idx;
  A.out_dist = (uint32_t *)out_dist;
  A.err = err;
  const int64_t ngroups = (nq + lsk::kBucket - 1) / lsk::kBucket;
  radius_walk_kernel<true><<<lsk_blocks(ngroups, kWaves), kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("radius_fill");
  return 0;
}

extern "C" int lsk_hip_radius_sort(const int64_t *offsets, int64_t nq, int64_t total, int64_t longest,
                                   int32_t *idx, float *dist, int sort, void *stream) {
  if (nq < 0 || total < 0 || longest < 0) {
    lsk::set_last_error("radius_sort: negative size");
    return 1;
  }
  if (nq == 0 || total == 0) return 0;
  if (!offsets || !idx || !dist) {
    lsk::set_last_error("radius_sort: null argument");
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  if (!sort) {
    radius_finalise_kernel<<<lsk_blocks(total, 256 * 4, 8192), 256, 0, st>>>((uint32_t *)dist, total);
    LSK_CHECK_LAUNCH("radius finalise");
    return 0;
  }
  radius_sort_lds_kernel<<<lsk_blocks(nq, kSortRows), kSortThreads, 0, st>>>(offsets, idx, (uint32_t *)dist, nq);
  LSK_CHECK_LAUNCH("radius sort");
  if (longest > (int64_t)kLdsRow) {
    radius_sort_big_kernel<<<lsk_blocks(nq, 1, 2048), kBigThreads, 0, st>>>(offsets, idx, (uint32_t *)dist, nq);
    LSK_CHECK_LAUNCH("radius sort (long rows)");
  }
  return 0;
}
