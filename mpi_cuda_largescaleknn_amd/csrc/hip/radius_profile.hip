// Radius profiles: for every query the number of points with d² < c_b at B ascending squared
// cutoffs c_0 <= ... <= c_{B-1} (strict, cumulative: column b is the count walk of radius.hip /
// periodic.hip at c_b, bit for bit), from one walk of the tree; and their sums over the queries,
// the pair counts S[b] of a two-point histogram, without the [nq, B] array. Weighted: the sum of
// the int64 weights of those points, WP[q, b], and WS[b] = sum over the queries of wq[q] * WP[q,
// b]. One walk kernel serves both; a policy (CountPolicy, WeightPolicy below) says what is added.
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
// n) to it without a distance evaluation and ignores the subtree (lsk::Cover). far >= cmax
// gives b0(far) = B != b0(near) < B: such a node is descended. With B = 1 this is the acceptance
// of radius.hip.
//
// Under a period near is image_point_dist2, the slackened gap that periodic.hip proves to be
// <= pd2 of every pair of the image inside the box, and the acceptance also requires both
// corners to take the image's wrap branch on all three axes (box_far of periodic_image.h, the
// test box_inside makes for one cutoff): every point of the node then belongs to this image
// for the lane and its pd2 is at most far. A candidate counts only in the image that is its
// wrap vector (`mine`), so each pair is counted once.
//
// Shell counters live in LDS, [wave][bin][lane] uint32: a wave's access to any mix of bins
// touches bank lane % 32 in each half-wave, conflict-free, and the update is one ds_add. Each
// lane owns its counters: no cross-lane atomics. 32 bins x 64 lanes x 4 B = 8 KB per wave, 32 KB
// per block beside the 5 KB of stacks and the cutoffs: four blocks (16 waves) share a CU's 160
// KB, the occupancy of the other walks.
//
// End of walk. Profile mode: each lane prefix-sums its shells and writes its row of the [nq,
// ld] array at the slice's column offset. Sum mode: the block adds every bin's shells over its
// 256 lanes (64-bit) and writes one row of [blocks, bins]; profile_reduce_kernel adds the rows
// and prefix-sums the bins. Integer sums: the result does not depend on the order.
//
// What the weight policy changes. The walk itself is untouched: the proof above is about WHICH
// shell a point falls in, not about what is added there, so both policies visit the same nodes,
// scan the same buckets and accept the same boxes (their stats are equal), and with every
// weight 1 the sums are the counts, bit for bit.
//  * The weights travel in curve order (wsorted[pos] = w[perm[pos]]): a bucket's 64 weights are
//    the scan's column (lsk::WeightCol), loaded one per lane beside the coordinates and
//    broadcast with them as two 32-bit readlanes. A candidate adds w to its shell.
//  * A node accepted whole adds wpre[p1] - wpre[p0] over its sorted positions [p0, p1)
//    (node_span, clipped at n), wpre [n + 1] being the exclusive prefix sum of wsorted: no
//    weight read per point.
//  * The counters are 64-bit: lane l's counter of a bin lies at dwords 2 l, 2 l + 1 of the
//    bin's 512-byte row, so the 8-byte accesses of any 16 consecutive lanes cover 32 distinct
//    banks and those of a 32-lane half 64 distinct banks, whatever mix of bins they address: by
//    that reasoning conflict-free under either banking rule of the LDS (and measured so:
//    SQ_LDS_BANK_CONFLICT is 0 for both policies, docs/ARCHITECTURE.md), and the update is one
//    64-bit ds_add. 16 bins x 64 lanes x 8 B is the same 8 KB per wave; hence 16 cutoffs per
//    launch (lsk_hip_weighted_profile_bins) against 32; longer lists run in slices, each
//    complete by itself.
//  * Sum mode first multiplies each lane's differential shells by its query's weight wq[row] (1
//    without wq).
//  * Exactness. The host admits only weights with max|w| * n < 2^62 and, for the pair sums,
//    (sum |w|) * (sum |wq|) < 2^63. Every sum formed here is a sum of a subset of the weights, or
//    of products wq * (such a sum) over a subset of the queries, so its true value lies within
//    those bounds; the arithmetic is wrapping 64-bit (unsigned), which is exact modulo 2^64
//    whatever the order and whatever the intermediate values (the prefix differences included),
//    so every result is the true value, and two runs give the same bits.
#include "periodic_image.h"

namespace {

using namespace lsk::periodic;

constexpr int kWaves = 4;  // waves per block, one query group each (as radius.hip)
constexpr int kReduceThreads = 256;

typedef unsigned long long u64;

struct ProfArgs {
  lsk_tree_view T;
  const float *qpts;         // sorted queries
  int64_t nq;
  const float *cut2s;        // [nb] ascending squared cutoffs (device)
  int32_t nb;                // 1 .. Policy::kBins
  float L[3];                // kPeriodic: the period
  const uint32_t *out_perm;  // sorted query -> query row
  const int64_t *wsorted;    // weights: [n] in curve order
  const int64_t *wpre;       // weights: [n + 1] exclusive prefix sum of wsorted
  const int64_t *wq;         // weights, sum: optional [nq] query weights, query order
  void *out;                 // profile: Policy::out_t [nq, ld], query order
  int64_t ld, col0;          // profile: row length and the slice's first column
  u64 *part;                 // sum: [gridDim.x, Policy::kBins] differential shell sums
  u64 *stats;                // optional [4] (kPeriodic: [5]), as radius.hip / periodic.hip
};

// What a profile adds up. counter: a shell counter (out_t: its signed form in the result);
// kBins: cutoffs per launch, 8 KB of counters per wave; column: what travels with a candidate
// through the scan, of(its value) what the candidate adds, node(A, p0, p1) what a node accepted
// whole adds for its sorted positions [p0, p1); factor(A, Q), where kQueryFactor, multiplies a
// lane's shells in sum mode.
struct CountPolicy {
  typedef uint32_t counter;
  typedef int32_t out_t;
  static constexpr int kBins = 32;
  static constexpr bool kWeights = false, kQueryFactor = false;
  static __device__ __forceinline__ lsk::NoCol column(const ProfArgs &) { return {}; }
  static __device__ __forceinline__ counter of(lsk::NoCol::value) { return 1u; }
  static __device__ __forceinline__ counter node(const ProfArgs &, int64_t p0, int64_t p1) {
    return (uint32_t)(p1 - p0);
  }
};

struct WeightPolicy {
  typedef u64 counter;
  typedef int64_t out_t;
  static constexpr int kBins = 16;
  static constexpr bool kWeights = true, kQueryFactor = true;
  static __device__ __forceinline__ lsk::WeightCol column(const ProfArgs &A) { return {A.wsorted}; }
  static __device__ __forceinline__ counter of(u64 w) { return w; }
  static __device__ __forceinline__ counter node(const ProfArgs &A, int64_t p0, int64_t p1) {
    return (u64)A.wpre[p1] - (u64)A.wpre[p0];
  }
  // (a lane without a query holds zeros)
  static __device__ __forceinline__ counter factor(const ProfArgs &A, const lsk::GroupQuery &Q) {
    return Q.valid ? (A.wq ? (u64)A.wq[Q.row] : 1ull) : 0ull;
  }
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

template <bool kPeriodic, bool kSum, class Policy>
__global__ __launch_bounds__(kWaves * 64) void radius_profile_walk_kernel(const ProfArgs A) {
  typedef typename Policy::counter counter;
  constexpr int kBins = Policy::kBins;
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  __shared__ counter shell_all[kWaves][kBins][64];
  __shared__ float cuts[kBins];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const uint32_t nb = (uint32_t)A.nb;
  if (threadIdx.x < (unsigned)kBins) cuts[threadIdx.x] = threadIdx.x < nb ? A.cut2s[threadIdx.x] : __builtin_inff();
  counter *shell = &shell_all[wid][0][0];
  for (uint32_t b = 0; b < nb; b++) shell[b * 64 + lane] = 0;
  __syncthreads();
  const float cmax = lsk::uniform_f(cuts[nb - 1]);
  const int steps = nb <= 1u ? 0 : 32 - __clz((int)(nb - 1u));
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  const bool active = g * lsk::kBucket < A.nq;  // (wave-uniform)
  lsk::GroupQuery Q{0, 0, 0.f, 0.f, 0.f, false, false};
  if (active) Q = lsk::load_group(g, lane, A.qpts, A.out_perm, A.nq);
  const bool live = Q.finite && cmax > 0.f;
  lsk::Cover cov;  // the whole node the lane took
  uint32_t s_evals = 0, s_accepts = 0, s_nodes = 0, s_buckets = 0, s_images = 0;
  const lsk_tree_view &T = A.T;

  // near < cmax. The whole node in one shell: add what the policy has for it there
  auto accept = [&](uint32_t node, int32_t lvl, uint32_t sp, float near, float far) {
    if (!(far < cmax)) return false;
    const uint32_t bf = shell_of(far, cuts, nb, steps);
    if (shell_of(near, cuts, nb, steps) != bf) return false;
    int64_t p0, p1;
    lsk::node_span(T, node, lvl, p0, p1);
    if (p1 > p0) atomicAdd(&shell[bf * 64 + lane], Policy::node(A, p0, p1));
    cov.take(sp);
    s_accepts++;
    return true;
  };
  // a bucket: the lanes that need it put its points into their shells one by one
  auto scan = [&](uint32_t node, bool use, const auto &diff) {
    const bool evals = use;
    const int cnt =
        lsk::scan_bucket(T, node, lane, Q, diff, Policy::column(A), lsk::NoCol{}, use, [&](const auto &c, bool &) {
          if (c.mine && c.d2 < cmax)
            atomicAdd(&shell[shell_of(c.d2, cuts, nb, steps) * 64 + lane], Policy::of(c.a));
        });
    if (cnt) s_buckets++;
    if (evals) s_evals += (uint32_t)cnt;
  };

  if (active && __ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    if (!kPeriodic) {
      const lsk::vec3f q{Q.x, Q.y, Q.z};
      lsk::ball_walk<true>(
          T, stk_all[wid], lane,
          [&](const float4 &lo4, const float4 &hi4) { return lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4)) < cmax; },
          [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
            s_nodes++;
            const float near = lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z});
            cov.pop(sp);
            bool use = live && near < cmax && !cov.on();
            if (use && accept(node, lvl, sp, near, lsk::far_dist2(Q.x, Q.y, Q.z, lo4, hi4))) use = false;
            return use;
          },
          [&](uint32_t node, bool use) { scan(node, use, lsk::OpenDiff{}); });
    } else {
      const Frame F = make_frame(T, A.L, gb);
      for (int im = 0; im < 27; im++) {  // (wave-uniform)
        Image I;
        if (!image_of(F.X, F.Y, F.Z, im, I)) continue;
        if (!(image_box_dist2(gb, F.rlo, F.rhi, I) < cmax)) continue;
        s_images++;
        cov.clear();
        lsk::ball_walk<true>(
            T, stk_all[wid], lane,
            [&](const float4 &lo4, const float4 &hi4) { return image_box_dist2(gb, lo4, hi4, I) < cmax; },
            [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
              s_nodes++;
              const float near = image_point_dist2(Q, lo4, hi4, I);
              cov.pop(sp);
              bool use = live && near < cmax && !cov.on();
              if (use) {
                float far;
                if (box_far(Q, lo4, hi4, F.X, F.Y, F.Z, I, far) && accept(node, lvl, sp, near, far)) use = false;
              }
              return use;
            },
            [&](uint32_t node, bool use) { scan(node, use, ImageDiff{F, I}); });
      }
    }
  }

  if (!kSum) {
    if (Q.valid) {
      typename Policy::out_t *row = (typename Policy::out_t *)A.out + Q.row * A.ld + A.col0;
      counter acc = 0;
      for (uint32_t b = 0; b < nb; b++) {
        acc += shell[b * 64 + lane];
        row[b] = (typename Policy::out_t)acc;
      }
    }
  } else {
    if constexpr (Policy::kQueryFactor) {
      const counter f = Policy::factor(A, Q);
      for (uint32_t b = 0; b < nb; b++) shell[b * 64 + lane] *= f;
    }
    __syncthreads();
    for (uint32_t b = (uint32_t)wid; b < nb; b += kWaves) {
      u64 v = 0;
      for (int w = 0; w < kWaves; w++) v += shell_all[w][b][lane];
      v = lsk::wave_sum64(v);
      if (lane == 0) A.part[(int64_t)blockIdx.x * kBins + b] = v;
    }
  }
  if (active)
    lsk::add_stats<kPeriodic>(A.stats, lane, s_evals, s_nodes, s_buckets, s_accepts, lane == 0 ? s_images : 0u);
}

// sums[col0 + b] = the sum over the rows of part[., 0 .. b]: the cumulative pair counts / sums.
template <int kBins>
__global__ __launch_bounds__(kReduceThreads) void profile_reduce_kernel(const u64 *__restrict__ part, int64_t nrows,
                                                                        int32_t nb, int64_t *__restrict__ sums,
                                                                        int64_t col0) {
  constexpr int kLanes = kReduceThreads / kBins;
  __shared__ u64 acc[kLanes][kBins];
  const int b = threadIdx.x % kBins, r0 = threadIdx.x / kBins;
  u64 s = 0;
  if (b < nb)
    for (int64_t r = r0; r < nrows; r += kLanes) s += part[r * kBins + b];
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

unsigned profile_blocks(int64_t nq) { return lsk_blocks((nq + lsk::kBucket - 1) / lsk::kBucket, kWaves); }

template <class Policy>
size_t sums_ws_bytes(int64_t nq) {
  return nq <= 0 ? 0 : (size_t)profile_blocks(nq) * Policy::kBins * sizeof(u64);
}

// The arguments every entry point shares (wsorted / wpre: of the weight policy only).
template <class Policy>
int profile_args(const char *what, const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *cut2s,
                 int32_t nb, const float *period, const uint32_t *out_perm, const int64_t *wsorted,
                 const int64_t *wpre, ProfArgs *A) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 32) || nb < 1 || nb > Policy::kBins) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)), "
                                            "0 <= nq < 2^32 or not 1 <= nb <= " + std::to_string(Policy::kBins));
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
  if (nq > 0 && (!qpts || !cut2s || !out_perm || (Policy::kWeights && (!wsorted || !wpre)))) {
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

template <class Policy>
int run_profile(const char *what, const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *cut2s,
                int32_t nb, const float *period, const uint32_t *out_perm, const int64_t *wsorted,
                const int64_t *wpre, void *out, int64_t ld, int64_t col0, u64 *stats, void *stream) {
  ProfArgs A;
  if (profile_args<Policy>(what, tree, qpts, nq, cut2s, nb, period, out_perm, wsorted, wpre, &A)) return 1;
  if (col0 < 0 || ld < col0 + nb) {
    lsk::set_last_error(std::string(what) + ": the slice [col0, col0 + nb) does not fit a row of ld columns");
    return 1;
  }
  if (nq == 0) return 0;
  if (!out) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  A.out = out;
  A.ld = ld;
  A.col0 = col0;
  A.stats = stats;
  const unsigned blocks = profile_blocks(nq);
  if (period)
    radius_profile_walk_kernel<true, false, Policy><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  else
    radius_profile_walk_kernel<false, false, Policy><<<blocks, kWaves * 64, 0, (hipStream_t)stream>>>(A);
  LSK_CHECK_LAUNCH(what);
  return 0;
}

template <class Policy>
int run_sums(const char *what, const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *cut2s,
             int32_t nb, const float *period, const uint32_t *out_perm, const int64_t *wsorted, const int64_t *wpre,
             const int64_t *wq, void *ws, int64_t *sums, int64_t col0, u64 *stats, void *stream) {
  ProfArgs A;
  if (profile_args<Policy>(what, tree, qpts, nq, cut2s, nb, period, out_perm, wsorted, wpre, &A)) return 1;
  if (col0 < 0) {
    lsk::set_last_error(std::string(what) + ": negative column offset");
    return 1;
  }
  if (nq == 0) return 0;
  if (!ws || !sums) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  A.wq = wq;
  A.part = (u64 *)ws;
  A.stats = stats;
  const unsigned blocks = profile_blocks(nq);
  hipStream_t st = (hipStream_t)stream;
  if (period)
    radius_profile_walk_kernel<true, true, Policy><<<blocks, kWaves * 64, 0, st>>>(A);
  else
    radius_profile_walk_kernel<false, true, Policy><<<blocks, kWaves * 64, 0, st>>>(A);
  LSK_CHECK_LAUNCH(what);
  profile_reduce_kernel<Policy::kBins><<<1, kReduceThreads, 0, st>>>(A.part, (int64_t)blocks, nb, sums, col0);
  LSK_CHECK_LAUNCH(std::string(what) + " (reduce)");
  return 0;
}

}  // namespace

extern "C" int lsk_hip_radius_profile_bins(void) { return CountPolicy::kBins; }

extern "C" int lsk_hip_radius_profile(const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *cut2s,
                                      int32_t nb, const float *period, const uint32_t *out_perm, int32_t *out,
                                      int64_t ld, int64_t col0, unsigned long long *stats, void *stream) {
  return run_profile<CountPolicy>("radius_profile", tree, qpts, nq, cut2s, nb, period, out_perm, nullptr, nullptr,
                                  out, ld, col0, stats, stream);
}

extern "C" size_t lsk_hip_pair_counts_ws_bytes(int64_t nq) { return sums_ws_bytes<CountPolicy>(nq); }

extern "C" int lsk_hip_pair_counts(const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *cut2s,
                                   int32_t nb, const float *period, const uint32_t *out_perm, void *ws,
                                   int64_t *sums, int64_t col0, unsigned long long *stats, void *stream) {
  return run_sums<CountPolicy>("pair_counts", tree, qpts, nq, cut2s, nb, period, out_perm, nullptr, nullptr,
                               nullptr, ws, sums, col0, stats, stream);
}

extern "C" int lsk_hip_weighted_profile_bins(void) { return WeightPolicy::kBins; }

extern "C" int lsk_hip_weighted_profile(const lsk_tree_view *tree, const float *qpts, int64_t nq,
                                        const float *cut2s, int32_t nb, const float *period,
                                        const uint32_t *out_perm, const int64_t *wsorted, const int64_t *wpre,
                                        int64_t *out, int64_t ld, int64_t col0, unsigned long long *stats,
                                        void *stream) {
  return run_profile<WeightPolicy>("weighted_profile", tree, qpts, nq, cut2s, nb, period, out_perm, wsorted, wpre,
                                   out, ld, col0, stats, stream);
}

extern "C" size_t lsk_hip_weighted_pair_sums_ws_bytes(int64_t nq) { return sums_ws_bytes<WeightPolicy>(nq); }

extern "C" int lsk_hip_weighted_pair_sums(const lsk_tree_view *tree, const float *qpts, int64_t nq,
                                          const float *cut2s, int32_t nb, const float *period,
                                          const uint32_t *out_perm, const int64_t *wsorted, const int64_t *wpre,
                                          const int64_t *wq, void *ws, int64_t *sums, int64_t col0,
                                          unsigned long long *stats, void *stream) {
  return run_sums<WeightPolicy>("weighted_pair_sums", tree, qpts, nq, cut2s, nb, period, out_perm, wsorted, wpre, wq,
                                ws, sums, col0, stats, stream);
}
