// Anisotropic pair counts: DD(rp, pi) and DD(s, mu) along a line of sight that is a box axis, as
// the cumulative int64 array of a 2-D two-point histogram, from one walk of the tree per slice of
// cells and without storing a pair.
//
// The contract. Per pair (dx, dy, dz) are the float32 per-axis differences q - p: in the open box
// those of lsk::OpenDiff, with a period the minimum image, literally wrap1 of periodic_image.h
// (one wrap vector per pair, no origin; a period of (inf, inf, inf) never wraps and equals the open
// box bit for bit). los in {0, 1, 2} picks the line-of-sight difference dl; the other two, in
// ascending axis order, are da and db. In float32, without contraction:
//     par2  = dl * dl
//     perp2 = fmaf(db, db, da * da)
//     d2    = the canonical dist2(dx, dy, dz)
// (rp, pi) mode, ascending cutoffs a2 = cp2[0 .. na), b2 = cl2[0 .. nb): the pair's cell is
//     i0 = #{i : !(perp2 < cp2[i])},  j0 = #{j : !(par2 < cl2[j])},
// and it is dropped when i0 == na or j0 == nb. Strict tests, negated: a NaN component passes no
// test, as in radius_profile.hip. The result is S[i, j] = #{pairs : perp2 < cp2[i] and par2 <
// cl2[j]}, the sum of the cells (i0 <= i, j0 <= j).
// (s, mu) mode, a2 = cs2 (squared s edges), b2 = mu2 (squared mu edges, each >= 0, inf allowed):
//     i0 = #{i : !(d2 < cs2[i])},  j0 = #{j : !(par2 < mu2[j] * d2)}      (one float32 product),
// dropped when out of range; S[i, j] = #{pairs : d2 < cs2[i] and par2 < mu2[j] * d2}. Two
// consequences: a pair with d2 == 0 (a self pair, exact copies) has 0 < 0 false (and 0 < NaN for
// an edge of inf) for every j and counts in no column; mu < 1 excludes the pairs that lie exactly
// along the line of sight, an edge of inf takes them in (par2 < inf for every d2 > 0). For d2 >=
// 0 the products mu2[j] * d2 ascend with j, so in both modes i0 and j0 are the first index whose
// test holds and a binary search finds them (first_of).
// A query with a NaN or infinite coordinate counts nothing: its non-finite component makes perp2,
// par2 or d2 non-finite (the kernel skips such a query; the result is the same).
//
// The walk has the shape of radius_profile_walk_kernel: 4 waves per block, one group of 64
// curve-consecutive queries per wave, the open walk or one walk per image the group can take;
// a candidate counts only in the image that is its wrap vector (`mine`), so each pair is counted
// once. The scan's difference (LosDiff) leaves par2 and perp2 beside the d2 it returns.
//
// Cull, (rp, pi) mode. A node is kept iff its perpendicular gap² < cp2[r1 - 1] and its
// line-of-sight gap² < cl2[nb - 1], the gap² being par / perp of the per-axis gaps of the group
// box (per lane: of the lane's own point) against the node's box. Open box: a per-axis gap is <=
// |fl(q - p)| for every p in the box (monotone float differences, the argument of box_dist2).
// Under a period the per-axis gaps are gap1 with its slack: the proof of periodic.hip ("The cull
// is conservative") bounds each axis by itself, max(0, fl(G - e_a)) <= |D_a| for every pair of the
// image inside the box, before anything is squared, so it holds for each component here. Squares
// and fma are monotone in their non-negative arguments: gap_perp2 <= perp2 and gap_par2 <= par2
// of every such pair, and a pair that counts has perp2 and par2 below the two cutoffs. Culling
// may add candidates, never drop one; the candidate test alone decides.
//
// Whole-box acceptance, (rp, pi) mode (proof). For a popped node a lane has near_perp2,
// near_par2 (the gaps above) and far_perp2, far_par2: par / perp of the per-axis larger |corner
// difference| (open box: as far_dist2; period: far1, the larger |wrapped corner difference|).
// Per-axis differences, squares and fma are monotone, so near_perp2 <= perp2 <= far_perp2 and
// near_par2 <= par2 <= far_par2 for every finite point of the box; under a period only when both
// corners take the image's wrap branch on all three axes (far1 on each: fl(q - p) is monotone in
// p and a branch is an interval, so every point between the corners takes it, belongs to this
// image for the lane, and d -> fl(d -+ L) being monotone its |wrapped difference| is at most the
// corner's). i0 and j0 are non-decreasing in their arguments: i0(near_perp2) <= i0(perp2) <=
// i0(far_perp2), likewise j0. When i0(near_perp2) == i0(far_perp2) < na and j0(near_par2) ==
// j0(far_par2) < nb every point of the node falls in that one cell: the lane adds the node's
// population (node_span, clipped at n) to it without a distance evaluation and covers the subtree
// (lsk::Cover). In a slice [r0, r1) of rows (below) the same holds for "below the slice": when
// both ends of the perpendicular range are < cp2[r0 - 1] no point of the node counts in this
// slice and the lane covers the subtree adding nothing.
//
// (s, mu) mode. The cull is the ball of cs2[r1 - 1], exactly that of the profile walk
// (box_box_dist2 / box_dist2, under a period image_box_dist2 / image_point_dist2). There is no
// whole-box acceptance: mu = |dl| / s is not monotone per axis, bounding it over a box needs the
// extremes of a ratio and separates cells only for boxes far smaller than their distance, where a
// bucket scan costs little; every pair inside the ball is evaluated.
//
// Counters. One block-shared LDS array of kCells = 2048 64-bit cells (16 KB, beside the 5 KB of
// stacks and the cutoffs), updated by the 64-bit LDS atomic add. 64-bit because a block's 256
// queries can put 256 n > 2^32 pairs into one cell. Every counting lane issues its own add. (A
// shortcut was measured and dropped: the counting lanes test by one ballot whether all hit the
// first one's cell and one lane adds their number. On a 20 x 40 (rp, pi) grid it cost 1.5 %, on
// a 20 x 20 (s, mu) grid it gained 1 %: docs/ARCHITECTURE.md.)
//
// Slices. A grid of more than kCells cells runs as slices of whole rows i0 in [r0, r1), all j,
// (r1 - r0) nb <= kCells, each complete by itself: a pair counts in the slice that holds its row.
//
// End of block. Every non-zero cell is added to the int64 [na, nb] result by one global 64-bit
// atomic add (the host zeroes the result first); there is no [blocks, cells] workspace. Integer
// sums: the result does not depend on the order, two runs give the same bits. A last small kernel
// turns the differential cells into the cumulative array in place.
//
// Weighted sums (lsk_hip_weighted_pair_sums_2d): WS[i, j] = the sum of wq[q] * w[p] over the pairs
// S[i, j] counts. The same kernel under a policy (CountPolicy, WeightPolicy below), as in
// radius_profile.hip; the walk is untouched, so both policies visit the same nodes, scan the same
// buckets and accept the same boxes (their stats are equal), and with every weight 1 the sums are
// the counts, bit for bit. Four places differ.
//  * Query weight: each lane loads wq[Q.row] once after load_group, as wrapping u64; 1 without wq.
//    The multiply by that 1 stays: a template flag that drops it would save no register the
//    allocation can use and the whole policy costs 4 - 12 % (docs/ARCHITECTURE.md), so the second
//    set of four instances was not built.
//  * Candidates: the weights travel in curve order as the scan's column (lsk::WeightCol, two
//    32-bit readlanes per point); a counting lane adds wq * w to its cell by the same 64-bit LDS
//    atomic add.
//  * Whole-box acceptance, (rp, pi): the lane adds wq * (wpre[p1] - wpre[p0]) over the node's
//    sorted positions [p0, p1) (node_span), wpre [n + 1] being the exclusive prefix sum of the
//    sorted weights: no weight read per point, no distance evaluation. The proof above is about
//    WHICH cell a point falls in, not about what is added there. "Below the slice" is unchanged.
//  * End of block and cumulate are the wrapping u64 adds they were (a cell whose weights cancel
//    to zero is skipped like an empty one).
// Exactness is that of radius_profile.hip ("What the weight policy changes"): the host admits only
// max|w| * n < 2^62 and (sum |w|) * (sum |wq|) < 2^63, every cell, partial sum and cumulative
// entry is a sum of wq * w over a subset of the pairs, so wrapping 64-bit arithmetic in any order
// gives the true value, and two runs give the same bits.
//
// Observer line of sight (lsk_hip_pair_counts_2d_observer, lsk_hip_weighted_pair_sums_2d_observer;
// kObserver, open box only). Every pair has its own line of sight, the direction from an observer
// o (three finite floats) to the pair's midpoint. Per pair, in float32 without contraction:
//     dx = q.x - p.x, dy, dz likewise            (the open-box difference above)
//     lx = (q.x - o.x) + (p.x - o.x), ly, lz     (twice the vector observer -> midpoint)
//     sl = fmaf(dz, lz, fmaf(dy, ly, dx * lx))
//     ll = dist2(lx, ly, lz),  d2 = dist2(dx, dy, dz)
//     par2  = (sl / ll) * sl                     (one correctly rounded division, one product)
//     perp2 = d2 - par2;  if (perp2 < 0) perp2 = 0     (a NaN stays a NaN)
// and the cells are those above: perp2 < cp2[i] and par2 < cl2[j], or d2 < cs2[i] and par2 <
// mu2[j] * d2. sl / ll has no dimension, so par2 is a squared length and the usable range of
// coordinates is that of d2. Swapping q and p negates sl exactly and leaves ll and d2 alone:
// every quantity is symmetric in its bits. A pair whose midpoint is the observer (ll == 0) has a
// NaN or infinite par2 and counts nowhere; a point with itself has par2 = perp2 = 0 (every (rp,
// pi) cell with cutoffs > 0, no (s, mu) cell); par2 may exceed d2 by rounding (perp2 clamps to 0;
// an edge mu = 1 excludes such a pair, inf takes it in). The difference functor ObsDiff is a
// sibling of LosDiff with q - o hoisted out of the candidate loop; row and column search, cell
// update, slices, end of block and cumulate are the ones above.
// Cull, observer mode. There is no axis: the cull is the ball box distance² < cull2 in both modes
// (box_box_dist2 / box_dist2, each <= the float d2 of every pair of the box, the proof of
// box_dist2). (s, mu): cull2 = cs2[r1 - 1]. (rp, pi): a pair that counts in the slice has
// fl(d2 - par2) < A (or that difference < 0 <= A) and par2 < B, with A = cp2[r1 - 1] and B =
// cl2[nb - 1]. Rounding to nearest is monotone and A is a float, so fl(x) < A implies x < A: the
// real d2 - par2 < A, and with par2 < B the float d2 < A + B as a real number. The host passes
// cull2 = nextafterf((float)((double)A + (double)B), +inf) >= A + B (the double sum of two floats
// is within one rounding of the real one, the float after its float rounding is above both), inf
// when either cutoff is: a node's box distance² <= d2 < cull2 for every pair that counts, so the
// cull drops none. There is no whole-box acceptance: neither component is monotone per axis under
// a per-pair direction (the argument given for mu above), the accept counter stays 0.
#include <algorithm>
#include <cmath>

#include "periodic_image.h"

namespace {

using namespace lsk::periodic;

constexpr int kWaves = 4;       // waves per block, one query group each (as radius_profile.hip)
constexpr int kCells = 2048;    // 64-bit LDS cells per block: a slice of the grid
constexpr int kMaxEdges = 2048; // cutoffs per axis
constexpr int kMaxGrid = 65536; // cells of the whole grid
constexpr int kCumThreads = 256;

typedef unsigned long long u64;

struct Pair2dArgs {
  lsk_tree_view T;
  const float *qpts;         // sorted queries
  int64_t nq;
  const float *a2, *b2;      // [na], [nb] ascending cutoffs of the two axes (device)
  int32_t na, nb;
  int32_t r0, r1;            // the slice: rows i0 in [r0, r1), (r1 - r0) * nb <= kCells
  int32_t los;               // 0, 1, 2
  float L[3];                // kPeriodic: the period
  const uint32_t *out_perm;  // sorted query -> query row
  u64 *out;                  // [na, nb] differential cells, zeroed by the host
  u64 *stats;                // optional [4] (kPeriodic: [5]), as radius_profile.hip
};

struct WeightedPair2dArgs : Pair2dArgs {
  const int64_t *wsorted;  // [n] point weights in curve order
  const int64_t *wpre;     // [n + 1] exclusive prefix sum of wsorted
  const int64_t *wq;       // optional [nq] query weights, query order
};

// kObserver: the policy's arguments and the observer's.
template <class Base>
struct ObserverArgs : Base {
  float o[3];   // the observer
  float cull2;  // the slice's ball: a node is kept iff its box distance² < cull2
};
template <class Policy, bool kObserver>
struct WalkArgs {
  typedef typename Policy::args type;
};
template <class Policy>
struct WalkArgs<Policy, true> {
  typedef ObserverArgs<typename Policy::args> type;
};

// What a pair adds to its cell. args: the kernel's argument block; column: what travels with a
// candidate through the scan; query(A, Q): the lane's factor, loaded once; of(f, its value): what
// a candidate adds; node(A, f, p0, p1): what a node accepted whole adds for its sorted positions
// [p0, p1).
struct CountPolicy {
  typedef Pair2dArgs args;
  static __device__ __forceinline__ lsk::NoCol column(const args &) { return {}; }
  static __device__ __forceinline__ u64 query(const args &, const lsk::GroupQuery &) { return 1ull; }
  static __device__ __forceinline__ u64 of(u64, lsk::NoCol::value) { return 1ull; }
  static __device__ __forceinline__ u64 node(const args &, u64, int64_t p0, int64_t p1) { return (u64)(p1 - p0); }
};

struct WeightPolicy {
  typedef WeightedPair2dArgs args;
  static __device__ __forceinline__ lsk::WeightCol column(const args &A) { return {A.wsorted}; }
  // (a lane without a query adds nothing anyway)
  static __device__ __forceinline__ u64 query(const args &A, const lsk::GroupQuery &Q) {
    return Q.valid && A.wq ? (u64)A.wq[Q.row] : 1ull;
  }
  static __device__ __forceinline__ u64 of(u64 f, u64 w) { return f * w; }
  static __device__ __forceinline__ u64 node(const args &A, u64 f, int64_t p0, int64_t p1) {
    return f * ((u64)A.wpre[p1] - (u64)A.wpre[p0]);
  }
};

// The three per-axis values ordered by the line of sight: (along, first other, second other).
__device__ __forceinline__ void by_los(int los, float x, float y, float z, float &l, float &a, float &b) {
  l = los == 0 ? x : (los == 1 ? y : z);
  a = los == 0 ? y : x;
  b = los == 2 ? y : z;
}
__device__ __forceinline__ float perp2_of(float a, float b) { return fmaf(b, b, a * a); }

// The difference of scan_bucket that also leaves par2 and perp2 of the pair in the lane's own
// variables: the open-box arithmetic of lsk::OpenDiff, or the minimum image and `mine` of ImageDiff.
template <bool kPeriodic>
struct LosDiff {
  const Frame *F;
  const Image *I;
  int los;
  float &par2, &perp2;
  __device__ __forceinline__ float operator()(const lsk::GroupQuery &Q, float x, float y, float z,
                                              bool &mine) const {
    float dx = Q.x - x, dy = Q.y - y, dz = Q.z - z;
    mine = true;
    if (kPeriodic) {
      int wx, wy, wz;
      dx = wrap1(dx, F->X.L, F->X.h, wx);
      dy = wrap1(dy, F->Y.L, F->Y.h, wy);
      dz = wrap1(dz, F->Z.L, F->Z.h, wz);
      mine = wx == I->x.s && wy == I->y.s && wz == I->z.s;
    }
    float dl, da, db;
    by_los(los, dx, dy, dz, dl, da, db);
    par2 = dl * dl;
    perp2 = perp2_of(da, db);
    return lsk::dist2(dx, dy, dz);
  }
};

// Its sibling for the observer line of sight (open box): the header's arithmetic, literally. qo =
// q - o is the lane's own, computed once before the walk.
struct ObsDiff {
  float ox, oy, oz;
  float qox, qoy, qoz;
  float &par2, &perp2;
  __device__ __forceinline__ float operator()(const lsk::GroupQuery &Q, float x, float y, float z,
                                              bool &mine) const {
    const float dx = Q.x - x, dy = Q.y - y, dz = Q.z - z;
    mine = true;
    const float lx = qox + (x - ox), ly = qoy + (y - oy), lz = qoz + (z - oz);
    const float sl = fmaf(dz, lz, fmaf(dy, ly, dx * lx));
    const float ll = lsk::dist2(lx, ly, lz);
    const float d2 = lsk::dist2(dx, dy, dz);
    par2 = __fdiv_rn(sl, ll) * sl;
    const float pp = d2 - par2;
    perp2 = pp < 0.f ? 0.f : pp;  // (a select, not fmaxf: a NaN stays a NaN)
    return d2;
  }
};

// The first index in [0, m) whose test holds, given that test(m - 1) holds and that the tests
// ascend (false ... false true ... true). `steps` = ceil(log2(m)), uniform.
template <class Test>
__device__ __forceinline__ uint32_t first_of(uint32_t m, int steps, Test test) {
  uint32_t lo = 0, hi = m - 1;
  for (int s = 0; s < steps; s++) {
    const uint32_t mid = (lo + hi) >> 1;
    const bool in = test(mid);
    hi = in ? mid : hi;
    lo = in ? lo : mid + 1;
  }
  return lo;
}

__device__ __forceinline__ int steps_of(uint32_t m) { return m <= 1u ? 0 : 32 - __clz((int)(m - 1u)); }

// Open-box per-axis gap of [qlo, qhi] against [lo, hi], and the larger |corner difference|.
__device__ __forceinline__ float open_gap(float qlo, float qhi, float lo, float hi) {
  return fmaxf(0.f, fmaxf(lo - qhi, qlo - hi));
}
__device__ __forceinline__ float open_far(float q, float lo, float hi) {
  return fmaxf(fabsf(lo - q), fabsf(hi - q));
}

// kSmu: (s, mu) mode, else (rp, pi). kObserver: the per-pair line of sight of an observer (open
// box), else the axis A.los.
template <bool kPeriodic, bool kSmu, class Policy, bool kObserver = false>
__global__ __launch_bounds__(kWaves * 64) void pair_counts_2d_walk_kernel(
    const typename WalkArgs<Policy, kObserver>::type A) {
  static_assert(!(kPeriodic && kObserver), "a periodic box has no observer");
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  __shared__ u64 cells[kCells];
  __shared__ float ca[kMaxEdges + 1];  // the slice's first-axis cutoffs, after the one below it
  __shared__ float cb[kMaxEdges];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const uint32_t nb = (uint32_t)A.nb;
  const uint32_t below = A.r0 > 0 ? 1u : 0u;           // ca[0] = a2[r0 - 1]: what is below the slice
  const uint32_t ma = (uint32_t)(A.r1 - A.r0) + below;  // entries of ca
  const uint32_t ncell = (uint32_t)(A.r1 - A.r0) * nb;  // <= kCells (the host checks)
  for (uint32_t i = threadIdx.x; i < ma; i += kWaves * 64) ca[i] = A.a2[(uint32_t)A.r0 - below + i];
  for (uint32_t i = threadIdx.x; i < nb; i += kWaves * 64) cb[i] = A.b2[i];
  for (uint32_t i = threadIdx.x; i < ncell; i += kWaves * 64) cells[i] = 0;
  __syncthreads();
  const float amax = lsk::uniform_f(ca[ma - 1]), bmax = lsk::uniform_f(cb[nb - 1]);
  const int sa = steps_of(ma), sb = steps_of(nb);
  const int los = A.los;
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  const bool active = g * lsk::kBucket < A.nq;  // (wave-uniform)
  lsk::GroupQuery Q{0, 0, 0.f, 0.f, 0.f, false, false};
  if (active) Q = lsk::load_group(g, lane, A.qpts, A.out_perm, A.nq);
  const bool live = Q.finite && amax > 0.f && bmax > 0.f;
  const u64 fq = Policy::query(A, Q);  // the lane's query weight
  lsk::Cover cov;  // the whole node the lane took
  uint32_t s_evals = 0, s_accepts = 0, s_nodes = 0, s_buckets = 0, s_images = 0;
  const lsk_tree_view &T = A.T;

  // row index within ca of a first-axis value v < amax; column of a par2 < bmax (rp, pi)
  auto row_of = [&](float v) { return first_of(ma, sa, [&](uint32_t i) { return v < ca[i]; }); };
  auto col_of = [&](float v) { return first_of(nb, sb, [&](uint32_t j) { return v < cb[j]; }); };
  // a counting lane (`on`) adds what the policy has for the candidate to its cell
  auto count = [&](bool on, uint32_t cell, auto w) {
    if (on) atomicAdd(&cells[cell], Policy::of(fq, w));
  };
  // (rp, pi): near_perp2 < amax, near_par2 < bmax. The whole node in one cell, or below the slice.
  auto accept = [&](uint32_t node, int32_t lvl, uint32_t sp, float np2, float nl2, float fp2, float fl2) {
    if (!(fp2 < amax) || !(fl2 < bmax)) return false;
    const uint32_t rf = row_of(fp2);
    if (row_of(np2) != rf) return false;
    if (rf >= below) {
      const uint32_t cf = col_of(fl2);
      if (col_of(nl2) != cf) return false;
      int64_t p0, p1;
      lsk::node_span(T, node, lvl, p0, p1);
      if (p1 > p0) atomicAdd(&cells[(rf - below) * nb + cf], Policy::node(A, fq, p0, p1));
    }
    cov.take(sp);
    s_accepts++;
    return true;
  };
  float par2 = 0.f, perp2 = 0.f;
  // a bucket: the lanes that need it put its points into their cells one by one
  auto scan = [&](uint32_t node, bool use, const auto &diff) {
    const bool evals = use;
    const int cnt = lsk::scan_bucket(T, node, lane, Q, diff, Policy::column(A), lsk::NoCol{}, use,
                                     [&](const auto &c, bool &) {
                                       const float va = kSmu ? c.d2 : perp2;
                                       bool on = c.mine && va < amax;
                                       uint32_t cell = 0;
                                       if (kSmu) {
                                         const float d2 = c.d2;
                                         on = on && par2 < bmax * d2;
                                         if (on) {
                                           const uint32_t r = row_of(va);
                                           const uint32_t j =
                                               first_of(nb, sb, [&](uint32_t k) { return par2 < cb[k] * d2; });
                                           on = r >= below;
                                           cell = (r - below) * nb + j;
                                         }
                                       } else {
                                         on = on && par2 < bmax;
                                         if (on) {
                                           const uint32_t r = row_of(va);
                                           on = r >= below;
                                           cell = (r - below) * nb + col_of(par2);
                                         }
                                       }
                                       count(on, cell, c.a);
                                     });
    if (cnt) s_buckets++;
    if (evals) s_evals += (uint32_t)cnt;
  };

  if (active && __ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    if constexpr (kObserver) {
      const lsk::vec3f q{Q.x, Q.y, Q.z};
      const float cull2 = A.cull2;
      const ObsDiff diff{A.o[0], A.o[1], A.o[2], Q.x - A.o[0], Q.y - A.o[1], Q.z - A.o[2], par2, perp2};
      lsk::ball_walk<true>(
          T, stk_all[wid], lane,
          [&](const float4 &lo4, const float4 &hi4) { return lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4)) < cull2; },
          [&](uint32_t, int32_t, uint32_t sp, const float4 &lo4, const float4 &hi4) {
            s_nodes++;
            cov.pop(sp);
            return live && lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}) < cull2;
          },
          [&](uint32_t node, bool use) { scan(node, use, diff); });
    } else if (!kPeriodic) {
      const lsk::vec3f q{Q.x, Q.y, Q.z};
      // (rp, pi): the two gap² of a query range against a box, both below their cutoffs
      auto near_ok = [&](float qlx, float qhx, float qly, float qhy, float qlz, float qhz, const float4 &lo4,
                         const float4 &hi4, float &np2, float &nl2) {
        float gl, ga, gbb;
        by_los(los, open_gap(qlx, qhx, lo4.x, hi4.x), open_gap(qly, qhy, lo4.y, hi4.y),
               open_gap(qlz, qhz, lo4.z, hi4.z), gl, ga, gbb);
        np2 = perp2_of(ga, gbb);
        nl2 = gl * gl;
        return np2 < amax && nl2 < bmax;
      };
      lsk::ball_walk<true>(
          T, stk_all[wid], lane,
          [&](const float4 &lo4, const float4 &hi4) {
            if (kSmu) return lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4)) < amax;
            float np2, nl2;
            return near_ok(gb.lo.x, gb.hi.x, gb.lo.y, gb.hi.y, gb.lo.z, gb.hi.z, lo4, hi4, np2, nl2);
          },
          [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
            s_nodes++;
            cov.pop(sp);
            if (kSmu)
              return live && lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z}) < amax;
            float np2, nl2;
            bool use = live && near_ok(Q.x, Q.x, Q.y, Q.y, Q.z, Q.z, lo4, hi4, np2, nl2) && !cov.on();
            if (use) {
              float fl, fa, fb;
              by_los(los, open_far(Q.x, lo4.x, hi4.x), open_far(Q.y, lo4.y, hi4.y), open_far(Q.z, lo4.z, hi4.z), fl,
                     fa, fb);
              if (accept(node, lvl, sp, np2, nl2, perp2_of(fa, fb), fl * fl)) use = false;
            }
            return use;
          },
          [&](uint32_t node, bool use) { scan(node, use, LosDiff<false>{nullptr, nullptr, los, par2, perp2}); });
    } else {
      const Frame F = make_frame(T, A.L, gb);
      for (int im = 0; im < 27; im++) {  // (wave-uniform)
        Image I;
        if (!image_of(F.X, F.Y, F.Z, im, I)) continue;
        auto near_ok = [&](float qlx, float qhx, float qly, float qhy, float qlz, float qhz, const float4 &lo4,
                           const float4 &hi4, float &np2, float &nl2) {
          float gl, ga, gbb;
          by_los(los, gap1(qlx, qhx, lo4.x, hi4.x, I.x), gap1(qly, qhy, lo4.y, hi4.y, I.y),
                 gap1(qlz, qhz, lo4.z, hi4.z, I.z), gl, ga, gbb);
          np2 = perp2_of(ga, gbb);
          nl2 = gl * gl;
          return np2 < amax && nl2 < bmax;
        };
        auto keep = [&](const float4 &lo4, const float4 &hi4) {
          if (kSmu) return image_box_dist2(gb, lo4, hi4, I) < amax;
          float np2, nl2;
          return near_ok(gb.lo.x, gb.hi.x, gb.lo.y, gb.hi.y, gb.lo.z, gb.hi.z, lo4, hi4, np2, nl2);
        };
        if (!keep(F.rlo, F.rhi)) continue;
        s_images++;
        cov.clear();
        lsk::ball_walk<true>(
            T, stk_all[wid], lane, keep,
            [&](uint32_t node, int32_t lvl, uint32_t sp, const float4 &lo4, const float4 &hi4) {
              s_nodes++;
              cov.pop(sp);
              if (kSmu) return live && image_point_dist2(Q, lo4, hi4, I) < amax;
              float np2, nl2;
              bool use = live && near_ok(Q.x, Q.x, Q.y, Q.y, Q.z, Q.z, lo4, hi4, np2, nl2) && !cov.on();
              if (use) {
                float fx, fy, fz;
                const bool in_x = far1(Q.x, lo4.x, hi4.x, F.X, I.x.s, fx), in_y = far1(Q.y, lo4.y, hi4.y, F.Y, I.y.s, fy),
                           in_z = far1(Q.z, lo4.z, hi4.z, F.Z, I.z.s, fz);
                float fl, fa, fb;
                by_los(los, fx, fy, fz, fl, fa, fb);
                if (in_x && in_y && in_z && accept(node, lvl, sp, np2, nl2, perp2_of(fa, fb), fl * fl)) use = false;
              }
              return use;
            },
            [&](uint32_t node, bool use) { scan(node, use, LosDiff<true>{&F, &I, los, par2, perp2}); });
      }
    }
  }

  __syncthreads();
  u64 *out = A.out + (int64_t)A.r0 * nb;
  for (uint32_t i = threadIdx.x; i < ncell; i += kWaves * 64) {
    const u64 v = cells[i];
    if (v) atomicAdd(&out[i], v);
  }
  if (active)
    lsk::add_stats<kPeriodic>(A.stats, lane, s_evals, s_nodes, s_buckets, s_accepts, lane == 0 ? s_images : 0u);
}

// Differential cells -> the cumulative [na, nb] array, in place, by one block: every row's running
// sum, then every column's.
__global__ __launch_bounds__(kCumThreads) void pair_counts_2d_cumulate_kernel(u64 *__restrict__ out, int32_t na,
                                                                               int32_t nb) {
  for (int32_t i = threadIdx.x; i < na; i += kCumThreads) {
    u64 run = 0;
    for (int32_t j = 0; j < nb; j++) {
      run += out[(int64_t)i * nb + j];
      out[(int64_t)i * nb + j] = run;
    }
  }
  __syncthreads();
  for (int32_t j = threadIdx.x; j < nb; j += kCumThreads) {
    u64 run = 0;
    for (int32_t i = 0; i < na; i++) {
      run += out[(int64_t)i * nb + j];
      out[(int64_t)i * nb + j] = run;
    }
  }
}

template <bool kPeriodic, class Policy, bool kObserver = false>
void launch_walk(const typename WalkArgs<Policy, kObserver>::type &A, bool smu, unsigned blocks, hipStream_t st) {
  if (smu)
    pair_counts_2d_walk_kernel<kPeriodic, true, Policy, kObserver><<<blocks, kWaves * 64, 0, st>>>(A);
  else
    pair_counts_2d_walk_kernel<kPeriodic, false, Policy, kObserver><<<blocks, kWaves * 64, 0, st>>>(A);
}

// What the entry points share: the argument checks, the zeroed result, one walk per slice of
// rows and the cumulate. A: the policy's arguments, its own fields set by the caller. kObserver:
// observer = three finite host floats, a2_host / b2_host = host copies of a2 / b2 (for the slices'
// cull2), los = 0 and period = null.
template <class Policy, bool kObserver = false>
int run_pairs_2d(const char *what, typename WalkArgs<Policy, kObserver>::type &A, const lsk_tree_view *tree,
                 const float *qpts, int64_t nq, const float *a2, int32_t na, const float *b2, int32_t nb,
                 int32_t mode, int32_t los, const float *period, const uint32_t *out_perm, int64_t *out,
                 unsigned long long *stats, void *stream, const float *observer = nullptr,
                 const float *a2_host = nullptr, const float *b2_host = nullptr) {
  if (!lsk_tree_ok(tree) || nq < 0 || nq >= ((int64_t)1 << 32) || na < 1 || na > kMaxEdges || nb < 1 ||
      nb > kMaxEdges || (int64_t)na * nb > kMaxGrid || mode < 0 || mode > 1 || los < 0 || los > 2) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n)), "
                                            "0 <= nq < 2^32, not 1 <= na, nb <= " + std::to_string(kMaxEdges) +
                        ", na * nb > " + std::to_string(kMaxGrid) + ", mode not 0 / 1 or los not 0 / 1 / 2");
    return 1;
  }
  for (int a = 0; a < 3; a++) {
    A.L[a] = period ? period[a] : __builtin_inff();
    if (!(A.L[a] > 0.f)) {
      lsk::set_last_error(std::string(what) + ": period must be three values > 0 (+inf: open axis)");
      return 1;
    }
  }
  if (!out || !a2 || !b2 || (nq > 0 && (!qpts || !out_perm)) || (kObserver && (!observer || !a2_host || !b2_host))) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  if constexpr (kObserver) {
    for (int a = 0; a < 3; a++) {
      A.o[a] = observer[a];
      if (!std::isfinite(A.o[a])) {
        lsk::set_last_error(std::string(what) + ": observer must be three finite values");
        return 1;
      }
    }
  }
  hipStream_t st = (hipStream_t)stream;
  LSK_HIP(lsk_fill32(out, 0u, (int64_t)na * nb * 2, st));
  if (nq == 0) return 0;
  A.T = *tree;
  A.qpts = qpts;
  A.nq = nq;
  A.a2 = a2;
  A.b2 = b2;
  A.na = na;
  A.nb = nb;
  A.los = los;
  A.out_perm = out_perm;
  A.out = (u64 *)out;
  A.stats = stats;
  const unsigned blocks = lsk_blocks((nq + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  const int32_t rows = kCells / nb;  // >= 1
  for (int32_t r0 = 0; r0 < na; r0 += rows) {
    A.r0 = r0;
    A.r1 = std::min(na, r0 + rows);
    if constexpr (kObserver) {
      // (rp, pi): the float after A + B (the header's proof); (s, mu): the slice's largest cs2
      const float top = a2_host[A.r1 - 1];
      A.cull2 = mode == 1 ? top : nextafterf((float)((double)top + (double)b2_host[nb - 1]), __builtin_inff());
      launch_walk<false, Policy, true>(A, mode == 1, blocks, st);
    } else if (period)
      launch_walk<true, Policy>(A, mode == 1, blocks, st);
    else
      launch_walk<false, Policy>(A, mode == 1, blocks, st);
    LSK_CHECK_LAUNCH(what);
  }
  pair_counts_2d_cumulate_kernel<<<1, kCumThreads, 0, st>>>(A.out, na, nb);
  LSK_CHECK_LAUNCH(std::string(what) + " (cumulate)");
  return 0;
}

}  // namespace

extern "C" int lsk_hip_pair_counts_2d_cells(void) { return kCells; }

// The one entry point (lsk_hip.h states the null rules): the policy from the weights, the walk from
// observer / period, `what` the name of that combination in error texts.
extern "C" int lsk_hip_pair_sums_2d(const lsk_tree_view *tree, const float *qpts, int64_t nq, const float *a2,
                                    const float *a2_host, int32_t na, const float *b2, const float *b2_host,
                                    int32_t nb, int32_t mode, int32_t los, const float *period,
                                    const float *observer, const uint32_t *out_perm, const int64_t *wsorted,
                                    const int64_t *wpre, const int64_t *wq, int64_t *out,
                                    unsigned long long *stats, void *stream) {
  const bool weighted = wsorted || wpre;
  const std::string what = std::string(weighted ? "weighted_pair_sums_2d" : "pair_counts_2d") +
                           (observer ? "_observer" : "");
  if (wq && !weighted) {
    lsk::set_last_error(what + ": query weights (wq) without point weights (wsorted, wpre)");
    return 1;
  }
  if (observer && period) {
    lsk::set_last_error(what + ": an observer line of sight takes no period (open box only)");
    return 1;
  }
  if (observer && (!a2_host || !b2_host)) {
    lsk::set_last_error(what + ": an observer line of sight needs the host copies a2_host and b2_host");
    return 1;
  }
  if (weighted && nq > 0 && (!wsorted || !wpre)) {
    lsk::set_last_error(what + ": null argument");
    return 1;
  }
  auto run = [&](auto policy, auto A) {
    using Policy = decltype(policy);
    constexpr bool kObserver = !std::is_same<decltype(A), typename Policy::args>::value;
    if constexpr (std::is_same<Policy, WeightPolicy>::value) {
      A.wsorted = wsorted;
      A.wpre = wpre;
      A.wq = wq;
    }
    return run_pairs_2d<Policy, kObserver>(what.c_str(), A, tree, qpts, nq, a2, na, b2, nb, mode, observer ? 0 : los,
                                           period, out_perm, out, stats, stream, observer, a2_host, b2_host);
  };
  if (weighted)
    return observer ? run(WeightPolicy{}, ObserverArgs<WeightedPair2dArgs>{})
                    : run(WeightPolicy{}, WeightedPair2dArgs{});
  return observer ? run(CountPolicy{}, ObserverArgs<Pair2dArgs>{}) : run(CountPolicy{}, Pair2dArgs{});
}
