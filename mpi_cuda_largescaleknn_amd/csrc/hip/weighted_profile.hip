// Weighted radius profiles: for every query the sum of the int64 weights of the points with d² <
// c_b at B ascending squared cutoffs (strict, cumulative), WP[q, b], from one walk of the tree;
// and WS[b] = sum over the queries of wq[q] * WP[q, b], the weighted pair sums of a two-point
// histogram, without the [nq, B] array. With every weight 1 these are the counts of
// radius_profile.hip, bit for bit.
//
// The walk is that of radius_profile.hip, open box and (kPeriodic) once per image: the same
// group cull, the same per-lane node test against cmax = c_{B-1}, the same shell b0(d²) = #{b :
// !(d² < c_b)} found by the same binary search, so the two kernels visit the same nodes, scan
// the same buckets and accept the same boxes (their stats are equal). Four things differ.
//
// Per-candidate weight. The weights travel in curve order (wsorted[pos] = w[perm[pos]]): a
// bucket's 64 weights are loaded one per lane beside the coordinates and broadcast with them as
// two 32-bit readlanes (scan_bucket_weight / scan_bucket_periodic_weight below, the scans of
// ball_walk.h / periodic_image.h with the weight in the functor). A lane adds w to the
// candidate's shell when d² < cmax; under a period only in the image that is the pair's wrap
// vector (`mine`), so each pair is added once.
//
// Whole-box acceptance. The proof in the header of radius_profile.hip is about WHICH shell a
// point of the node falls in (b0(near) <= b0(d²) <= b0(far); under a period with box_far's
// condition that the whole node belongs to the image), not about what is added there, so it
// carries over unchanged: when b0(near) == b0(far) the lane adds the node's weight to that one
// shell without a distance evaluation or a weight read. The node's weight is wpre[p1] -
// wpre[p0] over its sorted positions [p0, p1) (node_span, clipped at n), wpre [n + 1] being the
// exclusive prefix sum of wsorted.
//
// Exactness. The host admits only weights with max|w| * n < 2^62 and, for the pair sums, (sum
// |w|) * (sum |wq|) < 2^63. Every sum this file forms is a sum of a subset of the weights, or of
// products wq * (such a sum) over a subset of the queries, so its true value lies within those
// bounds; the arithmetic is wrapping 64-bit (unsigned), which is exact modulo 2^64 whatever the
// order and whatever the intermediate values (the prefix differences included), so every result
// is the true value. Integer sums: two runs give the same bits.
//
// Counters. The shell counters are 64-bit, in LDS as [wave][bin][lane]: lane l's counter of a
// bin lies at dwords 2 l, 2 l + 1 of the bin's 512-byte row, so the 8-byte accesses of any 16
// consecutive lanes cover 32 distinct banks and those of a 32-lane half 64 distinct banks,
// whatever mix of bins they address: by that reasoning conflict-free under either banking rule
// of the LDS (and measured so: SQ_LDS_BANK_CONFLICT is 0 for this kernel, as for
// radius_profile.hip's, docs/ARCHITECTURE.md), and the update is one 64-bit ds_add. Each lane
// owns its counters: no cross-lane atomics. 16 bins x 64 lanes x 8 B = 8 KB per wave, 32 KB per
// block of four waves beside the 5 KB of stacks and the cutoffs, the footprint of
// radius_profile.hip with its 32 bins of 4 bytes: four blocks (16 waves) share a CU's 160 KB,
// the occupancy of the other walks. Hence 16 cutoffs per launch
// (lsk_hip_weighted_profile_bins); longer lists run in slices, each complete by itself.
//
// End of walk. Profile mode: each lane prefix-sums its shells into its int64 row of [nq, ld] at
// the slice's column offset. Sum mode: each lane multiplies its differential shells by its
// query's weight wq[row] (1 without wq), the block adds every bin over its 256 lanes and writes
// one row of [blocks, kWeightedBins]; weighted_reduce_kernel adds the rows and prefix-sums the
// bins.
#include "periodic_image.h"

namespace {

using namespace lsk::periodic;

constexpr int kWaves = 4;          // waves per block, one query group each (as radius_profile.hip)
constexpr int kWeightedBins = 16;  // cutoffs per launch
constexpr int kReduceThreads = 256;

typedef unsigned long long u64;

struct WProfArgs {
  lsk_tree_view T;
  const float *qpts;         // sorted queries
  int64_t nq;
  const float *cut2s;        // [nb] ascending squared cutoffs (device)
  int32_t nb;                // 1 .. kWeightedBins
  float L[3];                // kPeriodic: the period
  const uint32_t *out_perm;  // sorted query -> query row
  const int64_t *wsorted;    // [n] weights in curve order
  const int64_t *wpre;       // [n + 1] exclusive prefix sum of wsorted
  const int64_t *wq;         // sum: optional [nq] query weights, query order
  int64_t *out;              // profile: [nq, ld], query order
  int64_t ld, col0;          // profile: row length and the slice's first column
  u64 *part;                 // sum: [gridDim.x, kWeightedBins] differential shell sums
  u64 *stats;                // optional [4] (kPeriodic: [5]), as radius_profile.hip
};

// shell_of of radius_profile.hip: b0(d2) for d2 < cuts[nb - 1], `steps` = ceil(log2(nb)).
__device__ __forceinline__ uint32_t shell_of(float d2, const float *cuts, uint32_t nb, int steps) {
  uint32_t lo = 0, hi = nb - 1;
  for (int s = 0; s < steps; s++) {
    const uint32_t mid = (lo + hi) >> 1;
    const bool in = d2 < cuts[mid];
    hi = in ? mid : hi;
    lo = in ? lo : mid + 1;
  }
  return lo;
}

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ u64 readlane_u64(uint32_t lo, uint32_t hi, int j) {
  const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)lo, j);
  const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)hi, j);
  return ((u64)h << 32) | (u64)l;
}

// scan_bucket of ball_walk.h with the candidates' weights (curve order) travelling beside
// them: cand(d2, weight of the point).
template <class Cand>
__device__ __forceinline__ int scan_bucket_weight(const lsk_tree_view &T, const int64_t *wsorted, uint32_t node,
                                                  int lane, const lsk::GroupQuery &Q, bool use, Cand cand) {
  const int64_t base = ((int64_t)node - ((int64_t)1 << T.depth)) * lsk::kBucket;
  if (base >= T.n) return 0;
  const int cnt = (int)min((int64_t)lsk::kBucket, T.n - base);
  const int64_t pi = base + lane;
  float px = 0.f, py = 0.f, pz = 0.f;
  uint32_t wl = 0, wh = 0;
  if (lane < cnt) {
    px = T.pts[3 * pi];
    py = T.pts[3 * pi + 1];
    pz = T.pts[3 * pi + 2];
    const u64 w = (u64)wsorted[pi];
    wl = (uint32_t)w;
    wh = (uint32_t)(w >> 32);
  }
  for (int j = 0; j < cnt; j++) {
    const float x = lsk::readlane_f(px, j), y = lsk::readlane_f(py, j), z = lsk::readlane_f(pz, j);
    const u64 w = readlane_u64(wl, wh, j);
    if (use) cand(lsk::dist2(Q.x - x, Q.y - y, Q.z - z), w);
  }
  return cnt;
}

// scan_bucket_periodic of periodic_image.h in the same way: cand(pd2, the pair's wrap vector is
// the image's, weight of the point).
template <class Cand>
__device__ __forceinline__ int scan_bucket_periodic_weight(const lsk_tree_view &T, const int64_t *wsorted,
                                                           uint32_t node, int lane, const lsk::GroupQuery &Q,
                                                           const Frame &F, const Image &I, bool use, Cand cand) {
  const int64_t base = ((int64_t)node - ((int64_t)1 << T.depth)) * lsk::kBucket;
  if (base >= T.n) return 0;
  const int cnt = (int)min((int64_t)lsk::kBucket, T.n - base);
  const int64_t pi = base + lane;
  float px = 0.f, py = 0.f, pz = 0.f;
  uint32_t wl = 0, wh = 0;
  if (lane < cnt) {
    px = T.pts[3 * pi];
    py = T.pts[3 * pi + 1];
    pz = T.pts[3 * pi + 2];
    const u64 w = (u64)wsorted[pi];
    wl = (uint32_t)w;
    wh = (uint32_t)(w >> 32);
  }
  for (int j = 0; j < cnt; j++) {
    const float x = lsk::readlane_f(px, j), y = lsk::readlane_f(py, j), z = lsk::readlane_f(pz, j);
    const u64 w = readlane_u64(wl, wh, j);
    if (use) {
      int wx, wy, wz;
      const float dx = wrap1(Q.x - x, F.X.L, F.X.h, wx), dy = wrap1(Q.y - y, F.Y.L, F.Y.h, wy),
                  dz = wrap1(Q.z - z, F.Z.L, F.Z.h, wz);
      cand(lsk::dist2(dx, dy, dz), wx == I.x.s && wy == I.y.s && wz == I.z.s, w);
    }
  }
  return cnt;
}

template <bool kPeriodic, bool kSum>
__global__ __launch_bounds__(kWaves * 64) void weighted_profile_walk_kernel(const WProfArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  __shared__ u64 shell_all[kWaves][kWeightedBins][64];
  __shared__ float cuts[kWeightedBins];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const uint32_t nb = (uint32_t)A.nb;
  if (threadIdx.x < (unsigned)kWeightedBins)
    cuts[threadIdx.x] = threadIdx.x < nb ? A.cut2s[threadIdx.x] : __builtin_inff();
  u64 *shell = &shell_all[wid][0][0];
  for (uint32_t b = 0; b < nb; b++) shell[b * 64 + lane] = 0ull;
  __syncthreads();
  const float cmax = lsk::uniform_f(cuts[nb - 1]);
  const int steps = nb <= 1u ? 0 : 32 - __clz((int)(nb - 1u));
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  const bool active = g * lsk::kBucket < A.nq;  // (wave-uniform)
  lsk::GroupQuery Q{0, 0, 0.f, 0.f, 0.f, false, false};
  if (active) Q = lsk::load_group(g, lane, A.qpts, A.out_perm, A.nq);
  const bool live = Q.finite && cmax > 0.f;
  // the lane took a whole node when the stack stood at cov_sp (radius.hip)
  bool cov = false;
  uint32_t cov_sp = 0;
  uint32_t s_evals = 0, s_accepts = 0, s_nodes = 0, s_buckets = 0, s_images = 0;

  auto add = [&](float d2, u64 w) {
    if (d2 < cmax) atomicAdd(&shell[shell_of(d2, cuts, nb, steps) * 64 + lane], w);
  };
  // near < cmax. The whole node in one shell: add its weight there
  auto accept = [&](const lsk_tree_view &T, uint32_t node, int32_t lvl, uint32_t sp, float near, float far) {
    if (!(far < cmax)) return false;
    const uint32_t bf = shell_of(far, cuts, nb, steps);
    if (shell_of(near, cuts, nb, steps) != bf) return false;
    int64_t p0, p1;
    lsk::node_span(T, node, lvl, p0, p1);
    if (p1 > p0) atomicAdd(&shell[bf * 64 + lane], (u64)A.wpre[p1] - (u64)A.wpre[p0]);
    cov = true;
    cov_sp = sp;
    s_accepts++;
    return true;
  };

  if (active && __ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    const lsk_tree_view &T = A.T;
    if (!kPeriodic) {
      const lsk::vec3f q{Q.x, Q.y, Q.z};
      lsk::ball_walk<true>(
          T, stk_all[wid], lane,
          [&](const float4 &lo4, const float4 &hi4) { return lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4)) < cmax; },
          [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
            s_nodes++;
            const float near = lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z});
            if (cov && sp < cov_sp) cov = false;
            bool use = live && near < cmax && !cov;
            if (use) {
              const float fx = fmaxf(fabsf(lo4.x - Q.x), fabsf(hi4.x - Q.x));
              const float fy = fmaxf(fabsf(lo4.y - Q.y), fabsf(hi4.y - Q.y));
              const float fz = fmaxf(fabsf(lo4.z - Q.z), fabsf(hi4.z - Q.z));
              if (accept(T, node, lvl, sp, near, lsk::dist2(fx, fy, fz))) use = false;
            }
            return use;
          },
          [&](uint32_t node, bool use) {
            const int cnt = scan_bucket_weight(T, A.wsorted, node, lane, Q, use, [&](float d2, u64 w) { add(d2, w); });
            if (cnt) s_buckets++;
            if (use) s_evals += (uint32_t)cnt;
          });
    } else {
      const Frame F = make_frame(T, A.L, gb);
      for (int im = 0; im < 27; im++) {  // (wave-uniform)
        Image I;
        if (!image_of(F.X, F.Y, F.Z, im, I)) continue;
        if (!(image_box_dist2(gb, F.rlo, F.rhi, I) < cmax)) continue;
        s_images++;
        cov = false;
        lsk::ball_walk<true>(
            T, stk_all[wid], lane,
            [&](const float4 &lo4, const float4 &hi4) { return image_box_dist2(gb, lo4, hi4, I) < cmax; },
            [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
              s_nodes++;
              const float near = image_point_dist2(Q, lo4, hi4, I);
              if (cov && sp < cov_sp) cov = false;
              bool use = live && near < cmax && !cov;
              if (use) {
                float far;
                if (box_far(Q, lo4, hi4, F.X, F.Y, F.Z, I, far) && accept(T, node, lvl, sp, near, far)) use = false;
              }
              return use;
            },
            [&](uint32_t node, bool use) {
              const int cnt = scan_bucket_periodic_weight(T, A.wsorted, node, lane, Q, F, I, use,
                                                          [&](float d2, bool mine, u64 w) {
                                                            if (mine) add(d2, w);
                                                          });
              if (cnt) s_buckets++;
              if (use) s_evals += (uint32_t)cnt;
            });
      }
    }
  }

  if (!kSum) {
    if (Q.valid) {
      int64_t *row = A.out + Q.row * A.ld + A.col0;
      u64 acc = 0;
      for (uint32_t b = 0; b < nb; b++) {
        acc += shell[b * 64 + lane];
        row[b] = (int64_t)acc;
      }
    }
  } else {
    // (a lane without a query holds zeros)
    const u64 wq = Q.valid ? (A.wq ? (u64)A.wq[Q.row] : 1ull) : 0ull;
    for (uint32_t b = 0; b < nb; b++) shell[b * 64 + lane] *= wq;
    __syncthreads();
    for (uint32_t b = (uint32_t)wid; b < nb; b += kWaves) {
      u64 v = 0;
      for (int w = 0; w < kWaves; w++) v += shell_all[w][b][lane];
      v = wave_sum64(v);
      if (lane == 0) A.part[(int64_t)blockIdx.x * kWeightedBins + b] = v;
    }
  }
  if (A.stats && active) {
    const uint32_t e = lsk::wave_sum(s_evals), a = lsk::wave_sum(s_accepts);
    if (lane == 0) {
      atomicAdd(&A.stats[0], (u64)e);
      atomicAdd(&A.stats[1], (u64)s_nodes);
      atomicAdd(&A.stats[2], (u64)s_buckets);
      atomicAdd(&A.stats[3], (u64)a);
      if (kPeriodic) atomicAdd(&A.stats[4], (u64)s_images);
    }
  }
}

// sums[col0 + b] = the sum over the rows of part[., 0 .. b]: the cumulative weighted pair sums.
__global__ __launch_bounds__(kReduceThreads) void weighted_reduce_kernel(const u64 *__restrict__ part, int64_t nrows,
                                                                         int32_t nb, int64_t *__restrict__ sums,
                                                                         int64_t col0) {
  constexpr int kLanes = kReduceThreads / kWeightedBins;
  __shared__ u64 acc[kLanes][kWeightedBins];
  const int b = threadIdx.x % kWeightedBins, r0 = threadIdx.x / kWeightedBins;
  u64 s = 0;
  if (b < nb)
    for (int64_t r = r0; r < nrows; r += kLanes) s += part[r * kWeightedBins + b];
  acc[r0][b] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 run = 0;
    for (int c = 0; c < nb; c++) {
      for (int k = 0; k < kLanes; k++) run += acc[k][c];
      sums[col0 + c] = (int64_t)run;
    }
  }
}

// The checks of radius_profile.hip's profile_args, and the weights.
int weighted_args(const char *what, const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *cut2s,
                  int32_t nb, const float *period, const uint32_t *out_perm, const int64_t *wsorted,
                  const int64_t *wpre, WProfArgs *A) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 32) || nb < 1 || nb > kWeightedBins) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)), "
                                            "0 <= nq < 2^32 or not 1 <= nb <= " + std::to_string(kWeightedBins));
    return 1;
  }
  *A = WProfArgs{};
  for (int a = 0; a < 3; a++) {
    A->L[a] = period ? period[a] : __builtin_inff();
    if (!(A->L[a] > 0.f)) {
      lsk::set_last_error(std::string(what) + ": period must be three values > 0 (+inf: open axis)");
      return 1;
    }
  }
  if (nq > 0 && (!qpts || !cut2s || !out_perm || !wsorted || !wpre)) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  A->T = *tree;
  A->qpts = qpts;
  A->nq = nq;
  A->cut2s = cut2s;
  A->nb = nb;
  A->out_perm = out_perm;
  A->wsorted = wsorted;
  A->wpre = wpre;
  return 0;
}

unsigned weighted_blocks(int64_t nq) { return lsk_blocks((nq + lsk::kBucket - 1) / lsk::kBucket, kWaves); }

}  // namespace

extern "C" int lsk_hip_weighted_profile_bins(void) { return kWeightedBins; }

extern "C" int lsk_hip_weighted_profile(const lsk_tree_view *tree, const float *qpts, int64_t nq,
                                        const float *cut2s, int32_t nb, const float *period,
                                        const uint32_t *out_perm, const int64_t *wsorted, const int64_t *wpre,
                                        int64_t *out, int64_t ld, int64_t col0, unsigned long long *stats,
                                        void *stream) {
  WProfArgs A;
  if (weighted_args("weighted_profile", tree, qpts, nq, cut2s, nb, period, out_perm, wsorted, wpre, &A)) return 1;
  if (col0 < 0 || ld < col0 + nb) {
    lsk::set_last_error("weighted_profile: the slice [col0, col0 + nb) does not fit a row of ld columns");
    return 1;
  }
  if (nq == 0) return 0;
  if (!out) {
    lsk::set_last_error("weighted_profile: null argument");
    return 1;
  }
  A.out = out;
  A.ld = ld;
  A.col0 = col0;
  A.stats = stats;
  const unsigned blocks = weighted_blocks(nq);
  if (period)
    weighted_profile_walk_kernel<true, false><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  else
    weighted_profile_walk_kernel<false, false><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("weighted_profile");
  return 0;
}

extern "C" size_t lsk_hip_weighted_pair_sums_ws_bytes(int64_t nq) {
  return nq <= 0 ? 0 : (size_t)weighted_blocks(nq) * kWeightedBins * sizeof(u64);
}

extern "C" int lsk_hip_weighted_pair_sums(const lsk_tree_view *tree, const float *qpts, int64_t nq,
                                          const float *cut2s, int32_t nb, const float *period,
                                          const uint32_t *out_perm, const int64_t *wsorted, const int64_t *wpre,
                                          const int64_t *wq, void *ws, int64_t *sums, int64_t col0,
                                          unsigned long long *stats, void *stream) {
  WProfArgs A;
  if (weighted_args("weighted_pair_sums", tree, qpts, nq, cut2s, nb, period, out_perm, wsorted, wpre, &A)) return 1;
  if (col0 < 0) {
    lsk::set_last_error("weighted_pair_sums: negative column offset");
    return 1;
  }
  if (nq == 0) return 0;
  if (!ws || !sums) {
    lsk::set_last_error("weighted_pair_sums: null argument");
    return 1;
  }
  A.wq = wq;
  A.part = (u64 *)ws;
  A.stats = stats;
  const unsigned blocks = weighted_blocks(nq);
  hipStream_t st = (hipStream_t)stream;
  if (period)
    weighted_profile_walk_kernel<true, true><<<blocks, kWaves * 64, 0, st>>>(A);
  else
    weighted_profile_walk_kernel<false, true><<<blocks, kWaves * 64, 0, st>>>(A);
  LSK_CHECK_LAUNCH("weighted_pair_sums");
  weighted_reduce_kernel<<<1, kReduceThreads, 0, st>>>(A.part, (int64_t)blocks, nb, sums, col0);
  LSK_CHECK_LAUNCH("weighted_pair_sums (reduce)");
  return 0;
}
