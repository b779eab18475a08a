// Radius profiles: for every query the number of points with d² < c_b at B ascending squared
// cutoffs c_0 <= ... <= c_{B-1} (strict, cumulative: column b is the count walk of radius.hip /
// periodic.hip at c_b, bit for bit), from one walk of the tree; and their sums over the queries,
// the pair counts S[b] of a two-point histogram, without the [nq, B] array.
//
// The walk is the count walk of radius.hip (kPeriodic: of periodic.hip, once per image) with
// cmax = c_{B-1} in the place of cut2: the group cull and the per-lane node test drop what is
// not nearer than cmax. What differs is where a point is counted. A lane keeps one counter
// per shell [c_{b-1}, c_b), differential, and a computed d² goes to shell
//     b0(d²) = #{b : !(d² < c_b)},
// dropped when b0 == B. The negated strict test keeps a NaN or infinite d² out of every shell
// (no comparison with it holds), as the strict test of radius.hip does; for the ascending
// cutoffs b0 is the first b with d² < c_b, found by a binary search (shell_of) once d² < cmax
// is known. Column b of the answer is the sum of the shells 0 .. b, taken at the end.
//
// Whole-box acceptance with many cutoffs (proof). For a popped node a lane has near =
// box_dist2(q, box) < cmax and far, the canonical dist2 of the per-axis larger corner
// difference. Per-axis float differences, squares and fma are monotone, so every finite point p
// inside the box has near <= d²(q, p) <= far (the argument of radius.hip, both ways), and b0 is
// non-decreasing in its argument: b0(near) <= b0(d²) <= b0(far). When b0(near) == b0(far) every
// point of the node falls in that one shell, so the lane adds the node's population (clipped at
// n) to it without a distance evaluation and ignores the subtree (cov / cov_sp as in
// radius.hip). far >= cmax gives b0(far) = B != b0(near) < B: such a node is descended. With B
// = 1 this is the acceptance of radius.hip.
//
// Under a period near is image_point_dist2, the slackened gap that periodic.hip proves to be
// <= pd2 of every pair of the image inside the box, and the acceptance also requires both
// corners to take the image's wrap branch on all three axes (box_far of periodic_image.h, the
// test box_inside makes for one cutoff): every point of the node then belongs to this image
// for the lane and its pd2 is at most far. A candidate counts only in the image that is its
// wrap vector, so each pair is counted once.
//
// Shell counters live in LDS, [wave][bin][lane] uint32: a wave's access to any mix of bins
// touches bank lane % 32 in each half-wave, conflict-free, and the update is one ds_add. 32
// bins x 64 lanes x 4 B = 8 KB per wave, 32 KB per block beside the 5 KB of stacks and the
// cutoffs: four blocks (16 waves) share a CU's 160 KB, the occupancy of the other walks.
//
// End of walk. Profile mode: each lane prefix-sums its shells and writes its row of the [nq,
// ld] array at the slice's column offset. Sum mode: the block adds every bin's shells over its
// 256 lanes (64-bit) and writes one row of [blocks, kProfileBins]; pair_reduce_kernel adds the
// rows and prefix-sums the bins. Integer sums: the result does not depend on the order.
#include "periodic_image.h"

namespace {

using namespace lsk::periodic;

constexpr int kWaves = 4;         // waves per block, one query group each (as radius.hip)
constexpr int kProfileBins = 32;  // cutoffs per launch
constexpr int kReduceThreads = 256;

struct ProfArgs {
  lsk_tree_view T;
  const float *qpts;         // sorted queries
  int64_t nq;
  const float *cut2s;        // [nb] ascending squared cutoffs (device)
  int32_t nb;                // 1 .. kProfileBins
  float L[3];                // kPeriodic: the period
  const uint32_t *out_perm;  // sorted query -> query row
  int32_t *out;              // profile: [nq, ld], query order
  int64_t ld, col0;          // profile: row length and the slice's first column
  unsigned long long *part;  // sum: [gridDim.x, kProfileBins] differential shell sums
  unsigned long long *stats; // optional [4] (kPeriodic: [5]), as radius.hip / periodic.hip
};

// b0(d2) for d2 < cuts[nb - 1]: the first b with d2 < cuts[b]. `steps` = ceil(log2(nb)),
// uniform; the range [lo, hi] keeps !(d2 < cuts[b]) for b < lo and d2 < cuts[hi].
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

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool kPeriodic, bool kSum>
__global__ __launch_bounds__(kWaves * 64) void radius_profile_walk_kernel(const ProfArgs A) {
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  __shared__ uint32_t shell_all[kWaves][kProfileBins][64];
  __shared__ float cuts[kProfileBins];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const uint32_t nb = (uint32_t)A.nb;
  if (threadIdx.x < (unsigned)kProfileBins)
    cuts[threadIdx.x] = threadIdx.x < nb ? A.cut2s[threadIdx.x] : __builtin_inff();
  uint32_t *shell = &shell_all[wid][0][0];
  for (uint32_t b = 0; b < nb; b++) shell[b * 64 + lane] = 0u;
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

  auto count = [&](float d2) {
    if (d2 < cmax) atomicAdd(&shell[shell_of(d2, cuts, nb, steps) * 64 + lane], 1u);
  };
  // near < cmax. The whole node in one shell: add its population there
  auto accept = [&](const lsk_tree_view &T, uint32_t node, int32_t lvl, uint32_t sp, float near, float far) {
    if (!(far < cmax)) return false;
    const uint32_t bf = shell_of(far, cuts, nb, steps);
    if (shell_of(near, cuts, nb, steps) != bf) return false;
    int64_t p0, p1;
    lsk::node_span(T, node, lvl, p0, p1);
    if (p1 > p0) atomicAdd(&shell[bf * 64 + lane], (uint32_t)(p1 - p0));
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
            const bool evals = use;
            const int cnt = lsk::scan_bucket<false>(T, nullptr, node, lane, Q, use,
                                                    [&](float d2, uint32_t, bool &) { count(d2); });
            if (cnt) s_buckets++;
            if (evals) s_evals += (uint32_t)cnt;
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
              const bool evals = use;
              const int cnt = scan_bucket_periodic<false, false>(
                  T, nullptr, nullptr, node, lane, Q, F, I, use,
                  [&](float d2, bool mine, uint32_t, uint32_t, uint32_t, bool &) {
                    if (mine) count(d2);
                  });
              if (cnt) s_buckets++;
              if (evals) s_evals += (uint32_t)cnt;
            });
      }
    }
  }

  if (!kSum) {
    if (Q.valid) {
      int32_t *row = A.out + Q.row * A.ld + A.col0;
      uint32_t acc = 0;
      for (uint32_t b = 0; b < nb; b++) {
        acc += shell[b * 64 + lane];
        row[b] = (int32_t)acc;
      }
    }
  } else {
    __syncthreads();
    for (uint32_t b = (uint32_t)wid; b < nb; b += kWaves) {
      unsigned long long v = 0;
      for (int w = 0; w < kWaves; w++) v += shell_all[w][b][lane];
      v = wave_sum64(v);
      if (lane == 0) A.part[(int64_t)blockIdx.x * kProfileBins + b] = v;
    }
  }
  if (A.stats && active) {
    const uint32_t e = lsk::wave_sum(s_evals), a = lsk::wave_sum(s_accepts);
    if (lane == 0) {
      atomicAdd(&A.stats[0], (unsigned long long)e);
      atomicAdd(&A.stats[1], (unsigned long long)s_nodes);
      atomicAdd(&A.stats[2], (unsigned long long)s_buckets);
      atomicAdd(&A.stats[3], (unsigned long long)a);
      if (kPeriodic) atomicAdd(&A.stats[4], (unsigned long long)s_images);
    }
  }
}

// sums[col0 + b] = the sum over the rows of part[., 0 .. b]: the cumulative pair counts.
__global__ __launch_bounds__(kReduceThreads) void pair_reduce_kernel(const unsigned long long *__restrict__ part,
                                                                     int64_t nrows, int32_t nb,
                                                                     int64_t *__restrict__ sums, int64_t col0) {
  constexpr int kLanes = kReduceThreads / kProfileBins;
  __shared__ unsigned long long acc[kLanes][kProfileBins];
  const int b = threadIdx.x % kProfileBins, r0 = threadIdx.x / kProfileBins;
  unsigned long long s = 0;
  if (b < nb)
    for (int64_t r = r0; r < nrows; r += kLanes) s += part[r * kProfileBins + b];
  acc[r0][b] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (int c = 0; c < nb; c++) {
      for (int k = 0; k < kLanes; k++) run += acc[k][c];
      sums[col0 + c] = (int64_t)run;
    }
  }
}

int profile_args(const char *what, const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *cut2s,
                 int32_t nb, const float *period, const uint32_t *out_perm, ProfArgs *A) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 32) || nb < 1 || nb > kProfileBins) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)), "
                                            "0 <= nq < 2^32 or not 1 <= nb <= " + std::to_string(kProfileBins));
    return 1;
  }
  *A = ProfArgs{};
  for (int a = 0; a < 3; a++) {
    A->L[a] = period ? period[a] : __builtin_inff();
    if (!(A->L[a] > 0.f)) {
      lsk::set_last_error(std::string(what) + ": period must be three values > 0 (+inf: open axis)");
      return 1;
    }
  }
  if (nq > 0 && (!qpts || !cut2s || !out_perm)) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  A->T = *tree;
  A->qpts = qpts;
  A->nq = nq;
  A->cut2s = cut2s;
  A->nb = nb;
  A->out_perm = out_perm;
  return 0;
}

unsigned profile_blocks(int64_t nq) { return lsk_blocks((nq + lsk::kBucket - 1) / lsk::kBucket, kWaves); }

}  // namespace

extern "C" int lsk_hip_radius_profile_bins(void) { return kProfileBins; }

extern "C" int lsk_hip_radius_profile(const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *cut2s,
                                      int32_t nb, const float *period, const uint32_t *out_perm, int32_t *out,
                                      int64_t ld, int64_t col0, unsigned long long *stats, void *stream) {
  ProfArgs A;
  if (profile_args("radius_profile", tree, qpts, nq, cut2s, nb, period, out_perm, &A)) return 1;
  if (col0 < 0 || ld < col0 + nb) {
    lsk::set_last_error("radius_profile: the slice [col0, col0 + nb) does not fit a row of ld columns");
    return 1;
  }
  if (nq == 0) return 0;
  if (!out) {
    lsk::set_last_error("radius_profile: null argument");
    return 1;
  }
  A.out = out;
  A.ld = ld;
  A.col0 = col0;
  A.stats = stats;
  const unsigned blocks = profile_blocks(nq);
  if (period)
    radius_profile_walk_kernel<true, false><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  else
    radius_profile_walk_kernel<false, false><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH("radius_profile");
  return 0;
}

extern "C" size_t lsk_hip_pair_counts_ws_bytes(int64_t nq) {
  return nq <= 0 ? 0 : (size_t)profile_blocks(nq) * kProfileBins * sizeof(unsigned long long);
}

extern "C" int lsk_hip_pair_counts(const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *cut2s,
                                   int32_t nb, const float *period, const uint32_t *out_perm, void *ws,
                                   int64_t *sums, int64_t col0, unsigned long long *stats, void *stream) {
  ProfArgs A;
  if (profile_args("pair_counts", tree, qpts, nq, cut2s, nb, period, out_perm, &A)) return 1;
  if (col0 < 0) {
    lsk::set_last_error("pair_counts: negative column offset");
    return 1;
  }
  if (nq == 0) return 0;
  if (!ws || !sums) {
    lsk::set_last_error("pair_counts: null argument");
    return 1;
  }
  A.part = (unsigned long long *)ws;
  A.stats = stats;
  const unsigned blocks = profile_blocks(nq);
  hipStream_t st = (hipStream_t)stream;
  if (period)
    radius_profile_walk_kernel<true, true><<<blocks, kWaves * 64, 0, st>>>(A);
  else
    radius_profile_walk_kernel<false, true><<<blocks, kWaves * 64, 0, st>>>(A);
  LSK_CHECK_LAUNCH("pair_counts");
  pair_reduce_kernel<<<1, kReduceThreads, 0, st>>>(A.part, (int64_t)blocks, nb, sums, col0);
  LSK_CHECK_LAUNCH("pair_counts (reduce)");
  return 0;
}
