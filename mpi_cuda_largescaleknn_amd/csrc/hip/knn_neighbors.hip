// Neighbour lists: ids and distances of all k nearest points of every query, collected
// from the exact k-th squared distance the k-th-distance kernels already found.
//
// Given the exact k-th value r of a query, its list is every point with d² < r (at most
// k - 1 by definition) plus enough of the points with d² == r to fill k slots, the lowest
// input rows first. No heap and no selection: one ball query per query group, appending
// straight into the output rows, then one in-place sort per row.
//
//  1. nb_collect_kernel: one wave owns 64 curve-consecutive sorted queries (lane = query).
//     It walks the bucket tree once for the group (wave-uniform DFS, 64-ary expansion,
//     stack in LDS, as knn_exact.hip::count_tree): a box is pruned when it is farther from
//     the group's box than the group's largest radius; a bucket is skipped by the lanes
//     whose own ball misses its box. A lane appends (d² bits, perm[pos]) of points below
//     its r from slot 0 upwards and ties from slot k - 1 downwards. front + back <= k
//     always: a tie that finds no free slot is dropped, a point below r that finds none
//     evicts the last tie. Ties are complete iff their count is <= k - below at the end;
//     otherwise (the choice among them matters: sorted order is curve order, not row
//     order) the query goes to the overflow list with `below` parked in its slot k - 1
//     (never a below-r slot: below <= k - 1).
//  2. nb_ties_kernel: wave per listed query, walks the tree for that query alone and keeps
//     the k - below smallest rows among the ties in a bounded LDS buffer that replaces its
//     maximum (correct for any number of exact copies; speed there is secondary).
//  3. nb_sort_kernel: bitonic sort of every row by (d² bits << 32 | id) in LDS, then
//     final_distance; unfilled slots (id -1, all-ones bits) sort last and get the cutoff.
//
// Safety: a row never receives more than k entries whatever r it was handed. A lane that
// sees more than k - 1 values below its r stops appending and bumps the error word, as
// does one that ends with fewer than k entries while r is below the cutoff. The host reads
// the word once after the pass; non-zero is a bug, not a fallback.
#include "dev.h"

namespace {

using lsk::bitsf;
using lsk::fbits;

constexpr int kWaves = 4;        // waves per block (collect: one query group each; ties: one query each)
constexpr int kStep = 6;         // levels per tree expansion (64 boxes, one per lane)
constexpr int kStack = 320;      // DFS stack entries per wave: 5 expansions x 63 siblings + 1
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

__device__ __forceinline__ float readlane_f(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  const float inf = __builtin_inff();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}

// Expand `node` (level lvl < depth) to its descendants min(kStep, depth - lvl) levels down:
// lane l < 2^step tests descendant l with `keep(child)`; the kept ones (that cover at
// least one bucket < nb) are pushed. Returns the new stack pointer.
template <class Keep>
__device__ __forceinline__ uint32_t expand(const float4 *nodes, uint32_t node, int32_t lvl, int32_t depth,
                                           int64_t nb, uint32_t *stk, uint32_t sp, int lane, Keep keep) {
  const int32_t step = min(kStep, depth - lvl);
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

__global__ __launch_bounds__(kWaves * 64) void nb_collect_kernel(const NbArgs A) {
  __shared__ uint32_t stk_all[kWaves][kStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  uint32_t *stk = stk_all[wid];
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= A.nq) return;  // (wave-uniform)
  const int64_t qi = g * lsk::kBucket + lane;
  const bool valid = qi < A.nq;
  const uint32_t k = A.k;
  const float inf = __builtin_inff();
  float qx = 0.f, qy = 0.f, qz = 0.f, r = -1.f;
  int64_t row = 0;
  if (valid) {
    qx = A.qpts[3 * qi];
    qy = A.qpts[3 * qi + 1];
    qz = A.qpts[3 * qi + 2];
    r = A.kth[qi];
    row = (int64_t)A.out_perm[qi] * k;
  }
  // a query with a non-finite coordinate has d² = inf or NaN to every point: no neighbours
  const bool live = valid && finite3(qx, qy, qz) && r >= 0.f;
  const bool tie_ok = live && r < A.cut2;  // r == cut2: fewer than k points qualify, no ties
  uint32_t front = 0, back = 0, ties = 0;
  bool bad = false;

  if (__ballot(live)) {
    const lsk::box3f gb{{lsk::wave_min(live ? qx : inf), lsk::wave_min(live ? qy : inf), lsk::wave_min(live ? qz : inf)},
                        {lsk::wave_max(live ? qx : -inf), lsk::wave_max(live ? qy : -inf),
                         lsk::wave_max(live ? qz : -inf)}};
    const float rmax = lsk::wave_max(live ? r : -1.f);
    const lsk::vec3f q{qx, qy, qz};
    const lsk_tree_view &T = A.T;
    const int32_t depth = T.depth;
    const int64_t nb = (T.n + lsk::kBucket - 1) / lsk::kBucket;
    const float4 *nodes = (const float4 *)T.nodes;
    uint32_t sp = 1;
    if (lane == 0) stk[0] = 1u;
    __builtin_amdgcn_wave_barrier();
    while (sp > 0) {
      sp--;
      const uint32_t node = lsk::uniform(stk[sp]);
      const int32_t lvl = 31 - __clz(node);
      if (lvl < depth) {
        sp = expand(nodes, node, lvl, depth, nb, stk, sp, lane, [&](const float4 &lo4, const float4 &hi4) {
          return lsk::box_box_dist2(gb, {{lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}}) <= rmax;
        });
        continue;
      }
      // a bucket: lanes whose ball reaches its box test its points one by one
      const int64_t base = ((int64_t)node - ((int64_t)1 << depth)) * lsk::kBucket;
      if (base >= T.n) continue;
      const int cnt = (int)min((int64_t)lsk::kBucket, T.n - base);
      const float4 lo4 = nodes[2 * node], hi4 = nodes[2 * node + 1];
      bool use = live && !bad && lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}) <= r;
      if (!__ballot(use)) continue;
      const int64_t pi = base + lane;
      float px = 0.f, py = 0.f, pz = 0.f;
      uint32_t pid = 0;
      if (lane < cnt) {
        px = T.pts[3 * pi];
        py = T.pts[3 * pi + 1];
        pz = T.pts[3 * pi + 2];
        pid = A.perm[pi];
      }
      for (int j = 0; j < cnt; j++) {
        const float x = readlane_f(px, j), y = readlane_f(py, j), z = readlane_f(pz, j);
        const uint32_t id = (uint32_t)__builtin_amdgcn_readlane((int)pid, j);
        if (use) {
          const float d2 = lsk::dist2(qx - x, qy - y, qz - z);
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
        }
      }
    }
  }

  if (bad) {
    atomicAdd(A.err, 1u);
    front = back = 0;
  }
  const uint32_t need = k - front;
  const bool ovf = live && !bad && ties > need;
  if (valid && !ovf) {
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
      A.ovf_list[e0 + __popcll(om & ((1ull << lane) - 1ull))] = (uint32_t)qi;
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
  __shared__ uint32_t stk_all[kWaves][kStack];
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
        sp = expand(nodes, node, lvl, depth, nb, stk, sp, lane, [&](const float4 &lo4, const float4 &hi4) {
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
      v = ((uint64_t)dist[o] << 32) | (uint32_t)idx[o];
    }
    key[e] = v;
  }
  __syncthreads();
  // bitonic network over every aligned kpad segment, all ascending
  for (uint32_t kk = 2; kk <= kpad; kk <<= 1) {
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < (uint32_t)kSortElems / 2; t += kSortThreads) {
        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
        const uint32_t p = i | j;
        const bool asc = ((i & (kpad - 1u)) & kk) == 0u;
        const uint64_t a = key[i], b = key[p];
        if ((a > b) == asc) {
          key[i] = b;
          key[p] = a;
        }
      }
      __syncthreads();
    }
  }
  const float fill = lsk::final_distance(cut2);
  for (uint32_t e = threadIdx.x; e < (uint32_t)kSortElems; e += kSortThreads) {
    const int64_t row = row0 + (e >> lg);
    const uint32_t c = e & (kpad - 1u);
    if (row < nq && c < k) {
      const int64_t o = row * k + c;
      const uint64_t v = key[e];
      const bool none = v == ~0ull;
      idx[o] = none ? -1 : (int32_t)(uint32_t)v;
      dist[o] = fbits(none ? fill : lsk::final_distance(bitsf((uint32_t)(v >> 32))));
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
  if (!tree || k < 1 || k > kMaxK || nq < 0 || nq >= ((int64_t)1 << 32)) {
    lsk::set_last_error("knn_neighbors: 1 <= k <= 1024, 0 <= nq < 2^32");
    return 1;
  }
  if (tree->n < 1 || tree->n >= ((int64_t)1 << 31) || tree->depth < 0 || tree->depth > 30 || !tree->nodes ||
      !tree->pts || lsk_hip_tree_depth(tree->n) != tree->depth) {
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
