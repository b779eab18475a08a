// Neighbour lists: ids and distances of all k nearest points of every query, collected
// from the exact k-th squared distance the k-th-distance kernels already found.
//
// Given the exact k-th value r of a query, its list is every point with d² < r (at most
// k - 1 by definition) plus enough of the points with d² == r to fill k slots, the lowest
// input rows first. No heap and no selection: one ball query per query group, appending
// straight into the output rows, then one in-place sort per row.
//
//  1. nb_collect_kernel: the group walk of ball_walk.h with every lane's own radius: a box
//     is pruned when it is farther from the group's box than the group's largest radius;
//     a bucket is skipped by the lanes whose own ball misses its box (inner nodes are not
//     tested per lane). A lane appends (d² bits, perm[pos]) of points below
//     its r from slot 0 upwards and ties from slot k - 1 downwards. front + back <= k
//     always: a tie that finds no free slot is dropped, a point below r that finds none
//     evicts the last tie. Ties are complete iff their count is <= k - below at the end;
//     otherwise (the choice among them matters: sorted order is curve order, not row
//     order) the query goes to the overflow list with `below` parked in its slot k - 1
//     (never a below-r slot: below <= k - 1).
//  2. nb_ties_kernel: wave per listed query, walks the tree for that query alone and keeps
//     the k - below smallest rows among the ties in a bounded LDS buffer that replaces its
//     maximum (correct for any number of exact copies; speed there is secondary).
//  3. nb_sort_kernel: every row sorted by (d² bits << 32 | id) in LDS (row_sort.h), then
//     final_distance; unfilled slots (id -1, all-ones bits) sort last and get the cutoff.
//
// Safety: a row never receives more than k entries whatever r it was handed. A lane that
// sees more than k - 1 values below its r stops appending and bumps the error word, as
// does one that ends with fewer than k entries while r is below the cutoff. The host reads
// the word once after the pass; non-zero is a bug, not a fallback.
#include "ball_walk.h"
#include "row_sort.h"

namespace {

using lsk::fbits;

constexpr int kWaves = 4;        // waves per block (collect: one query group each; ties: one query each)
constexpr int kMaxK = 1024;      // lsk_hip_knn_neighbors' limit (K.NEIGHBORS_MAX_K)
constexpr int kSortElems = 2048; // 64-bit keys per sort block (16 KB LDS): 2048 / kpad rows
constexpr int kSortThreads = 256;
constexpr uint32_t kNoDist = 0xffffffffu;  // d² bits of an unfilled slot (id -1)

struct NbArgs {
  lsk_tree_view T;
  const uint32_t *perm;      // sorted position -> input row
  const float *qpts;         // sorted queries
  const float *kth;          // their exact k-th d², sorted order
  int64_t nq;
  uint32_t k;
  float cut2;
  const uint32_t *out_perm;  // sorted query -> query row
  int32_t *out_idx;          // [nq][k]
  uint32_t *out_dist;        // [nq][k]: d² bits until the sort kernel finalises them
  uint32_t *err;
  uint32_t *ovf_list;        // [nq] sorted-order query indices whose ties overflowed
  uint32_t *ovf_count;
};

__global__ __launch_bounds__(kWaves * 64) void nb_collect_kernel(const NbArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= A.nq) return;  // (wave-uniform)
  const lsk::GroupQuery Q = lsk::load_group(g, lane, A.qpts, A.out_perm, A.nq);
  const uint32_t k = A.k;
  const float r = Q.valid ? A.kth[Q.qi] : -1.f;
  const int64_t row = Q.row * k;
  const bool live = Q.finite && r >= 0.f;
  const bool tie_ok = live && r < A.cut2;  // r == cut2: fewer than k points qualify, no ties
  uint32_t front = 0, back = 0, ties = 0;
  bool bad = false;

  if (__ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    const float rmax = lsk::wave_max(live ? r : -1.f);
    const lsk::vec3f q{Q.x, Q.y, Q.z};
    lsk::ball_walk<false>(
        A.T, stk_all[wid], lane,
        [&](const float4 &lo4, const float4 &hi4) { return lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4)) <= rmax; },
        // a bucket: lanes whose ball reaches its box test its points one by one
        [&](uint32_t, int32_t, uint32_t, const float4 &lo4, const float4 &hi4) {
          return live && !bad && lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}) <= r;
        },
        [&](uint32_t node, bool use) {
          lsk::scan_bucket(A.T, node, lane, Q, lsk::OpenDiff{}, lsk::Col<uint32_t>{A.perm}, lsk::NoCol{}, use,
                           [&](const auto &c, bool &use) {
            const float d2 = c.d2;
            const uint32_t id = c.a;
            if (d2 < r) {
              if (front + 1u >= k) {  // more than k - 1 values below the k-th: stop appending
                bad = true;
                use = false;
              } else {
                if (front + back == k) back--;  // the row is full: evict the last tie (it sits at `front`)
                A.out_idx[row + front] = (int32_t)id;
                A.out_dist[row + front] = fbits(d2);
                front++;
              }
            } else if (tie_ok && d2 == r) {
              ties++;
              if (front + back < k) {
                A.out_idx[row + (k - 1u - back)] = (int32_t)id;
                A.out_dist[row + (k - 1u - back)] = fbits(d2);
                back++;
              }
            }
          });
        });
  }

  if (bad) {
    atomicAdd(A.err, 1u);
    front = back = 0;
  }
  const uint32_t need = k - front;
  const bool ovf = live && !bad && ties > need;
  if (Q.valid && !ovf) {
    // (no overflow: back == ties <= need)
    if (tie_ok && !bad && ties < need) atomicAdd(A.err, 1u);  // fewer than k although r < cutoff
    for (uint32_t s = front; s < k - back; s++) {
      A.out_idx[row + s] = -1;
      A.out_dist[row + s] = kNoDist;
    }
  }
  const uint64_t om = __ballot(ovf);
  if (om) {
    uint32_t e0 = 0;
    if (lane == 0) e0 = atomicAdd(A.ovf_count, (uint32_t)__popcll(om));
    e0 = lsk::uniform(e0);
    if (ovf) {
      A.out_idx[row + k - 1u] = (int32_t)front;  // `below`, for nb_ties_kernel
      A.ovf_list[e0 + __popcll(om & ((1ull << lane) - 1ull))] = (uint32_t)Q.qi;
    }
  }
}

// Maximum of buf[0 .. m) and its position (uniform); m >= 1.
__device__ __forceinline__ void buf_max(const uint32_t *buf, uint32_t m, int lane, uint32_t &vmax, uint32_t &pmax) {
  uint32_t v = 0, p = 0;
  bool have = false;
  for (uint32_t t = lane; t < m; t += lsk::kWave) {
    const uint32_t b = buf[t];
    if (!have || b > v) {
      v = b;
      p = t;
      have = true;
    }
  }
  uint32_t mx = have ? v : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
  mx = lsk::uniform(mx);
  const uint64_t w = __ballot(have && v == mx);  // (ids are distinct; lane 0 always has one)
  const int src = (int)__builtin_ctzll(w);
  vmax = mx;
  pmax = lsk::uniform((uint32_t)__builtin_amdgcn_readlane((int)p, src));
}

__global__ __launch_bounds__(kWaves * 64) void nb_ties_kernel(const NbArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  __shared__ uint32_t buf_all[kWaves][kMaxK];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  uint32_t *stk = stk_all[wid];
  uint32_t *buf = buf_all[wid];
  const uint32_t k = A.k;
  const int64_t total = min((int64_t)A.ovf_count[0], A.nq);
  const lsk_tree_view &T = A.T;
  const int32_t depth = T.depth;
  const int64_t nb = (T.n + lsk::kBucket - 1) / lsk::kBucket;
  const float4 *nodes = (const float4 *)T.nodes;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wid; i < total; i += (int64_t)gridDim.x * kWaves) {
    const int64_t qi = (int64_t)lsk::uniform(A.ovf_list[i]);
    if (qi >= A.nq) continue;
    const float qx = lsk::uniform_f(A.qpts[3 * qi]);
    const float qy = lsk::uniform_f(A.qpts[3 * qi + 1]);
    const float qz = lsk::uniform_f(A.qpts[3 * qi + 2]);
    const float r = lsk::uniform_f(A.kth[qi]);
    const int64_t row = (int64_t)lsk::uniform(A.out_perm[qi]) * k;
    const uint32_t below = lsk::uniform((uint32_t)A.out_idx[row + k - 1u]);
    if (below >= k) {  // (not what nb_collect_kernel writes)
      if (lane == 0) atomicAdd(A.err, 1u);
      for (uint32_t s = lane; s < k; s += lsk::kWave) {
        A.out_idx[row + s] = -1;
        A.out_dist[row + s] = kNoDist;
      }
      continue;
    }
    const uint32_t need = k - below;  // 1 .. k <= kMaxK
    const lsk::vec3f q{qx, qy, qz};
    uint32_t c = 0, vmax = 0, pmax = 0;  // buffer fill, its maximum and where it sits (uniform)
    uint32_t sp = 1;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) stk[0] = 1u;
    __builtin_amdgcn_wave_barrier();
    while (sp > 0) {
      sp--;
      const uint32_t node = lsk::uniform(stk[sp]);
      const int32_t lvl = 31 - __clz(node);
      if (lvl < depth) {
        sp = lsk::expand(nodes, node, lvl, depth, nb, stk, sp, lane, [&](const float4 &lo4, const float4 &hi4) {
          return lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}) <= r;
        });
        continue;
      }
      const int64_t pi = ((int64_t)node - ((int64_t)1 << depth)) * lsk::kBucket + lane;
      bool tie = false;
      uint32_t id = 0;
      if (pi < T.n) {
        tie = lsk::dist2(qx - T.pts[3 * pi], qy - T.pts[3 * pi + 1], qz - T.pts[3 * pi + 2]) == r;
        if (tie) id = A.perm[pi];
      }
      // candidates one by one (a full buffer admits only rows below its maximum)
      uint64_t m = __ballot(tie && (c < need || id < vmax));
      while (m) {
        const int j = (int)__builtin_ctzll(m);
        m &= m - 1ull;
        const uint32_t idj = (uint32_t)__builtin_amdgcn_readlane((int)id, j);
        if (c < need) {
          if (lane == 0) buf[c] = idj;
          c++;
          if (c < need) continue;
        } else if (idj < vmax) {
          if (lane == 0) buf[pmax] = idj;
        } else {
          continue;
        }
        __builtin_amdgcn_wave_barrier();
        buf_max(buf, need, lane, vmax, pmax);
        __builtin_amdgcn_wave_barrier();
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (c < need && lane == 0) atomicAdd(A.err, 1u);  // the collect pass counted more ties than exist
    for (uint32_t s = lane; s < need; s += lsk::kWave) {
      A.out_idx[row + below + s] = s < c ? (int32_t)buf[s] : -1;
      A.out_dist[row + below + s] = s < c ? fbits(r) : kNoDist;
    }
  }
}

// Rows [blockIdx * R, +R), R = kSortElems / kpad, each padded to kpad = 2^lg keys.
__global__ __launch_bounds__(kSortThreads) void nb_sort_kernel(int32_t *__restrict__ idx, uint32_t *__restrict__ dist,
                                                               int64_t nq, uint32_t k, uint32_t lg, float cut2) {
  __shared__ uint64_t key[kSortElems];
  const uint32_t kpad = 1u << lg;
  const int64_t row0 = (int64_t)blockIdx.x * (kSortElems >> lg);
  for (uint32_t e = threadIdx.x; e < (uint32_t)kSortElems; e += kSortThreads) {
    const int64_t row = row0 + (e >> lg);
    const uint32_t c = e & (kpad - 1u);
    uint64_t v = ~0ull;
    if (row < nq && c < k) {
      const int64_t o = row * k + c;
      v = lsk::pack_key(dist[o], idx[o]);
    }
    key[e] = v;
  }
  __syncthreads();
  lsk::sort_rows_lds(key, kSortElems, kpad, kSortThreads);
  const uint32_t fill = fbits(lsk::final_distance(cut2));
  for (uint32_t e = threadIdx.x; e < (uint32_t)kSortElems; e += kSortThreads) {
    const int64_t row = row0 + (e >> lg);
    const uint32_t c = e & (kpad - 1u);
    if (row < nq && c < k) {
      const int64_t o = row * k + c;
      const uint64_t v = key[e];
      const bool none = v == ~0ull;
      idx[o] = none ? -1 : lsk::key_id(v);
      dist[o] = none ? fill : lsk::finalised(lsk::key_d2bits(v));
    }
  }
}

}  // namespace

extern "C" size_t lsk_hip_knn_neighbors_ws_bytes(int64_t nq) {
  return (size_t)(nq < 0 ? 0 : nq) * 4 + 256;
}

extern "C" int lsk_hip_knn_neighbors(const lsk_tree_view *tree, const uint32_t *perm, const float *qpts,
                                     const float *kth_d2, int64_t nq, int32_t k, float cut2,
                                     const uint32_t *out_perm, int32_t *out_idx, float *out_dist, uint32_t *err,
                                     void *ws, void *stream) {
  if (k < 1 || k > kMaxK || nq < 0 || nq >= ((int64_t)1 << 32)) {
    lsk::set_last_error("knn_neighbors: 1 <= k <= 1024, 0 <= nq < 2^32");
    return 1;
  }
  if (!lsk_tree_ok(tree)) {
    lsk::set_last_error("knn_neighbors: tree view incomplete (1 <= n < 2^31, depth = tree_depth(n))");
    return 1;
  }
  if (nq == 0) return 0;
  if (!perm || !qpts || !kth_d2 || !out_perm || !out_idx || !out_dist || !err || !ws) {
    lsk::set_last_error("knn_neighbors: null argument");
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  NbArgs A;
  A.T = *tree;
  A.perm = perm;
  A.qpts = qpts;
  A.kth = kth_d2;
  A.nq = nq;
  A.k = (uint32_t)k;
  A.cut2 = cut2;
  A.out_perm = out_perm;
  A.out_idx = out_idx;
  A.out_dist = (uint32_t *)out_dist;
  A.err = err;
  A.ovf_count = (uint32_t *)ws;  // 64 words, then the list
  A.ovf_list = (uint32_t *)ws + 64;
  LSK_HIP(lsk_fill32(A.ovf_count, 0u, 1, st));
  const int64_t ngroups = (nq + lsk::kBucket - 1) / lsk::kBucket;
  nb_collect_kernel<<<lsk_blocks(ngroups, kWaves), kWaves * 64, 0, st>>>(A);
  LSK_CHECK_LAUNCH("knn_neighbors collect");
  // persistent, device-counted: an empty overflow list costs one short launch
  nb_ties_kernel<<<lsk_blocks(nq, kWaves, 1024), kWaves * 64, 0, st>>>(A);
  LSK_CHECK_LAUNCH("knn_neighbors ties");
  uint32_t lg = 0;
  while ((1u << lg) < (uint32_t)k) lg++;
  const int64_t rows_per_block = kSortElems >> lg;
  nb_sort_kernel<<<lsk_blocks(nq, (int)rows_per_block), kSortThreads, 0, st>>>(out_idx, (uint32_t *)out_dist, nq,
                                                                            (uint32_t)k, lg, cut2);
  LSK_CHECK_LAUNCH("knn_neighbors sort");
  return 0;
}
