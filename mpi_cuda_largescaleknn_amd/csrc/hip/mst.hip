// Euclidean minimum spanning tree over one index by Boruvka rounds on the bucket tree, and the
// edge hook that turns a sorted edge list back into friends-of-friends labels.
//
// The contract: vertices are the finite points; the weight of {a, b} is w = dist2(a, b), or with
// core distances w = max(dist2(a, b), core[a], core[b]) (the max of floats is exact); the key
// of an edge is (bits of w, lo, hi) with lo < hi the two input rows, compared lexicographically.
// That is a strict total order, so the MST is unique and the result below is the oracle's edge
// set whatever the number of rounds or the order in which atomics land.
//
// Everything works in sorted positions, as in cluster.hip: a wave owns one bucket (lane =
// point). The state is O(n): parent / comp (union-find forest and its flattened roots), best
// (per point), cmin / chi (per component, at its root position), ncomp (per tree node). A round:
//
//  1. mst_comp_kernel     comp[pos] = root of pos (the smallest position of its component: unite
//     hooks the larger root under the smaller), kWild for a point with a NaN or infinite
//     coordinate, which is no vertex. Own launch: every unite of the round before is visible.
//  2. mst_leaf_kernel, mst_level_kernel   ncomp[node] = the component that all finite points of
//     the node share, kMixed where there are several, kNone where there is no finite point.
//     Buckets by a wave reduction, inner levels bottom-up, one launch per level as tree.hip.
//  3. mst_nearest_kernel  per finite point q the smallest (bits of w << 32 | input row of p)
//     over the points p of other components. For a fixed q, ordering the candidates by (w,
//     row_p) equals ordering the pairs by (w, lo, hi): with equal w and row_p1 < row_p2, both
//     above row_q give lo = row_q twice and hi in that order; both below give lo in that order;
//     row_p1 < row_q < row_p2 gives lo = row_p1 < row_q = lo of the second. So 64 bits suffice.
//     A node is dropped for a lane when ncomp[node] is the lane's own component (nothing
//     foreign inside) or when the bits of max(box_dist2(q, box), core[q]) exceed the bits of
//     the lane's best w: no point inside has a smaller w (common.h: box_dist2 is a lower bound
//     of the computed dist2; w >= core[q]). Equality is kept: a tie may bring a lower row.
//     The walk is nearest-first along the curve instead of one DFS from the root, whose lanes
//     would start without a bound: the wave's own bucket, its two curve neighbours, then the
//     subtree of the sibling of every ancestor of the bucket from the deepest up. The bucket and
//     those siblings partition the tree, so the walk is complete.
//  4. mst_min1_kernel, mst_min2_kernel   per component the smallest full key: atomicMin of
//     (bits of w << 32 | lo) at cmin[comp], then atomicMin of hi at chi[comp] among the points
//     whose first part matches. Minima over integers: order-independent.
//  5. mst_emit_kernel     the one point of a component whose candidate has the component's
//     key (one: the other end of the pair is foreign) writes the edge to a counter-allocated
//     slot and unites the two positions, unless the partner component chose the same edge and
//     has the smaller id (then that one writes). The slots' order is irrelevant: the caller
//     sorts by key.
// Every component picks its smallest outgoing edge under a strict total order, so the picked
// edges are MST edges, form no cycle, and the components at least halve per round.
//
// Under a period (lsk_hip_mst_periodic_round) the weight of a pair is pd2, the minimum image of
// periodic.hip, symmetric in its bits, and only step 3 changes (mst_nearest_periodic_kernel,
// whose second argument MstPeriod carries the period). Every pair has exactly one wrap vector in {-1, 0, +1}^3, and the
// walk visits the images one after the other; a candidate counts in the image that is its wrap
// vector (`mine` of ImageDiff) and nowhere else, so the minimum over images is the minimum over
// pairs. The 64-bit key argument above does not ask which image a pair came from.
//   Image 0 first, in the open order and under the open culls: a pair of wrap vector 0 has pd2 =
//   the open-box dist2 bit for bit, of which box_dist2 / box_box_dist2 are lower bounds as before.
//   After it nearly every lane holds a bound.
//   Then every other image the group can take (image_of), one ball walk from the root each, the
//   boxes tested against the shifted query by the slackened gaps image_box_dist2 (group) and
//   image_point_dist2 (lane). periodic.hip proves that these are lower bounds of pd2 for every
//   pair of the image inside the box ("The cull is conservative"); that proof argues per pair and
//   never uses cut2 <= fl(h h): only the whole-box acceptance and the tight nodes of periodic.hip
//   need that bound, and the nearest walk has neither, so an edge may be as long as it likes and
//   the coordinates need not lie inside one period. A node is dropped for a lane as in image 0:
//   ncomp[node] its own component (nothing foreign inside, whatever the shift), or the bits of
//   max(gap, core[q]) above its best w; equality is kept.
//   What image 0 knows does not carry over: the own bucket and the two curve neighbours are
//   ordinary buckets of a shifted walk (their pairs with that wrap vector were not counted in
//   image 0; with n <= 64 every wrapped pair is such a pair), and a lane may arrive without any
//   candidate (every foreign point wraps): maxbw is then all ones and the walk runs unbounded.
//   The image loop and maxbw are wave-uniform; every walk starts and ends with an empty stack, so
//   the kWalkStack words of a wave serve all of them. L = inf never wraps and takes no image but
//   0: an open period gives the open result bit for bit.
//
// As in cluster.hip no lane waits on another lane, wave or flag, and no loop is unbounded:
// unite's retries strictly lower a position, a parent chain strictly decreases (a chain that
// does not bumps the error word and gives up: the host raises), and every tree walk pops a
// stack that each expansion can only fill with descendants.
#include <type_traits>

#include "cluster_uf.h"
#include "periodic_image.h"

namespace {

using namespace lsk::periodic;
using lsk::fbits;
using lsk::load_own;
using lsk::unite;

constexpr int kWaves = 4;                  // waves per block, one bucket each (as cluster.hip)
constexpr uint32_t kWild = 0xffffffffu;    // comp[]: no vertex (a NaN or infinite coordinate)
constexpr uint32_t kMixed = 0xffffffffu;   // ncomp[]: finite points of more than one component
constexpr uint32_t kNone = 0xfffffffeu;    // ncomp[]: no finite point
constexpr unsigned long long kNoKey = ~0ull;

// The nearest walk pushes nothing beyond kWalkStack's proof: every sub-walk starts at a node of
// the tree with an empty stack and ends with an empty stack, and walk_stack bounds the stack of
// a walk from the root, of which a walk from any other node is the tail.
static_assert(lsk::kWalkStack == lsk::walk_stack(lsk::kWalkStep) && lsk::kWalkStack >= (1 << lsk::kWalkStep) + 1,
              "one stack of kWalkStack words per wave serves the own-bucket scan and every sibling walk");

struct MstArgs {
  lsk_tree_view T;
  const uint32_t *perm;        // sorted position -> input row
  const float *core;           // optional [n]: core distances (squared), sorted positions
  uint32_t *parent;            // [n]
  uint32_t *comp;              // [n]
  uint32_t *ncomp;             // [2^(depth + 1)]
  unsigned long long *best;    // [n] (bits of w << 32 | row of the nearest foreign point)
  uint32_t *best_pos;          // [n] that point's sorted position
  unsigned long long *cmin;    // [n] at a root: (bits of w << 32 | lo) of the component's edge
  uint32_t *chi;               // [n] at a root: hi of the component's edge
  int32_t *erows;              // [n][2] edges: (lo, hi)
  float *ew;                   // [n] edges: w
  uint32_t *count;             // edges written so far
  uint32_t *err;
  unsigned long long *stats;   // optional [5]: distance evaluations, nodes popped, buckets scanned, image
                               // walks beyond image 0 (periodic), CAS retries
};

// What the nearest walk knows about the box. OpenBox: nothing, the difference of a scan is the
// open one. PeriodicBox: the period (the kernel's second argument), the group's frame and image 0.
struct OpenBox {
  static constexpr bool kPeriodic = false;
  __device__ __forceinline__ void init(const lsk_tree_view &, const lsk::box3f &) {}
  __device__ __forceinline__ lsk::OpenDiff diff0() const { return {}; }
};
struct PeriodicBox {
  static constexpr bool kPeriodic = true;
  float L[3];
  Frame F;
  Image I0;
  __device__ __forceinline__ void init(const lsk_tree_view &T, const lsk::box3f &gb) {
    F = make_frame(T, L, gb);
    image_of(F.X, F.Y, F.Z, 13, I0);
  }
  __device__ __forceinline__ ImageDiff diff0() const { return {F, I0}; }
};
struct MstPeriod {
  float L[3];
};

__device__ __forceinline__ uint32_t wave_min_u(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// The two integer columns a candidate of the nearest walk carries: its component and its row.
struct CompRowCol {
  struct value {
    uint32_t comp, row;
  };
  const uint32_t *comp, *perm;
  uint32_t c = 0, r = 0;
  __device__ __forceinline__ void load(int64_t pi) {
    c = comp[pi];
    r = perm[pi];
  }
  __device__ __forceinline__ value get(int j) const {
    return {(uint32_t)__builtin_amdgcn_readlane((int)c, j), (uint32_t)__builtin_amdgcn_readlane((int)r, j)};
  }
};

__global__ __launch_bounds__(256) void mst_comp_kernel(const MstArgs A) {
  const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= A.T.n) return;
  uint32_t x = kWild;
  if (lsk::finite3(A.T.pts[3 * pos], A.T.pts[3 * pos + 1], A.T.pts[3 * pos + 2])) {
    const uint32_t n = (uint32_t)A.T.n;
    uint32_t steps = 0;
    x = (uint32_t)pos;
    for (uint32_t p = A.parent[x]; p != x; p = A.parent[x]) {
      if (p > x || ++steps > n) {  // (never: see find)
        atomicAdd(A.err, 1u);
        break;
      }
      x = p;
    }
    // (an ancestor of pos, not above the value that was there: unite's invariants hold)
    if (x < (uint32_t)pos) atomicMin(A.parent + pos, x);
  }
  A.comp[pos] = x;
  A.cmin[pos] = kNoKey;
  A.chi[pos] = 0xffffffffu;
}

__global__ __launch_bounds__(kWaves * 64) void mst_leaf_kernel(const MstArgs A) {
  const int lane = lsk::lane_id();
  const int64_t b = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= ((int64_t)1 << A.T.depth)) return;  // (wave-uniform)
  const int64_t pos = b * lsk::kBucket + lane;
  const uint32_t c = pos < A.T.n ? A.comp[pos] : kWild;
  const uint32_t mn = wave_min_u(c);
  const bool mixed = __ballot(c != kWild && c != mn) != 0;
  if (lane == 0) A.ncomp[((int64_t)1 << A.T.depth) + b] = mn == kWild ? kNone : mixed ? kMixed : mn;
}

__global__ __launch_bounds__(256) void mst_level_kernel(const MstArgs A, int level) {
  const int64_t cnt = (int64_t)1 << level;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cnt) return;
  const int64_t node = cnt + j;
  const uint32_t a = A.ncomp[2 * node], b = A.ncomp[2 * node + 1];
  uint32_t v;
  if (a == kNone)
    v = b;
  else if (b == kNone || a == b)
    v = a;
  else
    v = kMixed;
  A.ncomp[node] = v;
}

template <bool kCore, class Box>
__device__ __forceinline__ void mst_nearest(const MstArgs &A, Box &B) {
  constexpr bool kPeriodic = Box::kPeriodic;
  __shared__ uint32_t stk_all[kWaves][lsk::kWalkStack];
  const int wid = threadIdx.x >> 6;
  const int lane = lsk::lane_id();
  const lsk_tree_view &T = A.T;
  const int64_t g = (int64_t)blockIdx.x * kWaves + wid;
  if (g * lsk::kBucket >= T.n) return;  // (wave-uniform)
  const lsk::GroupQuery Q = load_own(T, g, lane);
  const bool live = Q.finite;
  const uint32_t pos_q = (uint32_t)Q.qi;
  const uint32_t cq = live ? A.comp[pos_q] : kNone;  // (kNone: no candidate's and no node's value a lane could share)
  float kq = 0.f;
  if (kCore && live) kq = A.core[pos_q];
  unsigned long long best = kNoKey;
  uint32_t best_pos = 0;
  uint32_t s_evals = 0, s_nodes = 0, s_buckets = 0, s_images = 0;
  if (__ballot(live)) {
    const lsk::box3f gb = lsk::group_box(Q, live);
    const lsk::vec3f q{Q.x, Q.y, Q.z};
    const int32_t depth = T.depth;
    const int64_t nb = (T.n + lsk::kBucket - 1) / lsk::kBucket;
    const uint32_t leaf = ((uint32_t)1 << depth) + (uint32_t)g;
    // the two curve neighbours, scanned before the walk and not again (0: none)
    const uint32_t left = g > 0 ? leaf - 1 : 0u, right = g + 1 < nb ? leaf + 1 : 0u;
    // (wave-uniform) the largest bound of the live lanes, as bits; all ones while a lane has none
    uint32_t maxbw = 0xffffffffu;
    using CoreCol = std::conditional_t<kCore, lsk::FloatCol, lsk::NoCol>;
    // the bucket scan of a walk under the difference of its image (open box: every candidate is
    // `mine`). A maker and not one more call level around the scan: the open form then compiles
    // to the code it had before there was a periodic one.
    auto scan_under = [&](const auto diff) {
      return [&, diff](uint32_t node, bool use) {
        const bool evals = use;
        CoreCol cc{};
        if constexpr (kCore) cc.p = A.core;
        const int cnt = lsk::scan_bucket(T, node, lane, Q, diff, CompRowCol{A.comp, A.perm}, cc, use,
                                         [&](const auto &c, bool &) {
                                           if (c.mine && c.a.comp != cq && c.a.comp != kWild) {
                                             float w = c.d2;
                                             if constexpr (kCore) w = fmaxf(fmaxf(w, kq), c.b);
                                             const unsigned long long key = ((unsigned long long)fbits(w) << 32) | c.a.row;
                                             if (key < best) {
                                               best = key;
                                               best_pos = c.pos;
                                             }
                                           }
                                         });
        if (cnt) s_buckets++;
        if (evals) s_evals += (uint32_t)cnt;
        maxbw = wave_max_u(live ? (uint32_t)(best >> 32) : 0u);
      };
    };
    // image 0: the pairs of wrap vector 0, whose pd2 is the open-box dist2, in the open order
    // and under the open culls
    B.init(T, gb);
    auto on_bucket = scan_under(B.diff0());
    on_bucket(leaf, live);
    if (left) on_bucket(left, live);
    if (right) on_bucket(right, live);
    auto keep = [&](const float4 &lo4, const float4 &hi4) {
      return fbits(lsk::box_box_dist2(gb, lsk::box_of(lo4, hi4))) <= maxbw;
    };
    auto on_node = [&](uint32_t node, int32_t, uint32_t, const float4 &lo4, const float4 &hi4) {
      s_nodes++;
      const uint32_t nc = A.ncomp[node];  // (wave-uniform)
      float bd2 = lsk::box_dist2(q, {lo4.x, lo4.y, lo4.z}, {hi4.x, hi4.y, hi4.z});
      if (kCore) bd2 = fmaxf(bd2, kq);
      return live && nc != kNone && nc != cq && node != left && node != right &&
             fbits(bd2) <= (uint32_t)(best >> 32);
    };
    for (int32_t lvl = depth; lvl >= 1; lvl--) {
      const uint32_t sib = (leaf >> (depth - lvl)) ^ 1u;
      const int64_t first = ((int64_t)sib - ((int64_t)1 << lvl)) << (depth - lvl);
      if (first >= nb) continue;  // (covers no bucket: its slot of the node array is not a box)
      lsk::ball_walk_from<true>(T, stk_all[wid], lane, sib, keep, on_node, on_bucket);
    }
    if constexpr (kPeriodic) {
      // every other image the group can take, one walk from the root each: the own bucket and
      // the curve neighbours are ordinary buckets here, and a lane may still have no bound
      const Frame &F = B.F;
      for (int im = 0; im < 27; im++) {  // (wave-uniform)
        Image I;
        if (im == 13 || !image_of(F.X, F.Y, F.Z, im, I)) continue;
        if (fbits(image_box_dist2(gb, F.rlo, F.rhi, I)) > maxbw) continue;
        s_images++;
        lsk::ball_walk<true>(
            T, stk_all[wid], lane,
            [&](const float4 &lo4, const float4 &hi4) { return fbits(image_box_dist2(gb, lo4, hi4, I)) <= maxbw; },
            [&](uint32_t node, int32_t, uint32_t, const float4 &lo4, const float4 &hi4) {
              s_nodes++;
              const uint32_t nc = A.ncomp[node];  // (wave-uniform)
              float bd2 = image_point_dist2(Q, lo4, hi4, I);
              if (kCore) bd2 = fmaxf(bd2, kq);
              return live && nc != kNone && nc != cq && fbits(bd2) <= (uint32_t)(best >> 32);
            },
            scan_under(ImageDiff{F, I}));
      }
    }
  }
  if (Q.valid) {
    A.best[pos_q] = best;
    A.best_pos[pos_q] = best_pos;
  }
  lsk::add_stats<false>(A.stats, lane, s_evals, s_nodes, s_buckets, lane == 0 ? s_images : 0u);
}

template <bool kCore>
__global__ __launch_bounds__(kWaves * 64) void mst_nearest_kernel(const MstArgs A) {
  OpenBox B;
  mst_nearest<kCore>(A, B);
}

template <bool kCore>
__global__ __launch_bounds__(kWaves * 64) void mst_nearest_periodic_kernel(const MstArgs A, const MstPeriod P) {
  PeriodicBox B;
  B.L[0] = P.L[0];
  B.L[1] = P.L[1];
  B.L[2] = P.L[2];
  mst_nearest<kCore>(A, B);
}

// The first two fields of the lane's candidate edge (bits of w << 32 | lo) and the third.
struct EdgeKey {
  bool act;
  uint32_t comp, hi;
  unsigned long long wlo;
};

__device__ __forceinline__ EdgeKey edge_key(const MstArgs &A, int64_t pos) {
  EdgeKey e{false, 0u, 0u, kNoKey};
  if (pos >= A.T.n) return e;
  const unsigned long long b = A.best[pos];
  if (b == kNoKey) return e;
  const uint32_t rq = A.perm[pos], rp = (uint32_t)b;
  e.act = true;
  e.comp = A.comp[pos];
  e.hi = max(rq, rp);
  e.wlo = (b & 0xffffffff00000000ull) | (unsigned long long)min(rq, rp);
  return e;
}

// A lane whose key is not below the value already there (a hint: the value only decreases) sends
// no atomic: a large component costs a few, not one per point.
__global__ __launch_bounds__(256) void mst_min1_kernel(const MstArgs A) {
  const EdgeKey e = edge_key(A, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  if (e.act && e.wlo < A.cmin[e.comp]) atomicMin(A.cmin + e.comp, e.wlo);
}

__global__ __launch_bounds__(256) void mst_min2_kernel(const MstArgs A) {
  const EdgeKey e = edge_key(A, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  if (e.act && e.wlo == A.cmin[e.comp] && e.hi < A.chi[e.comp]) atomicMin(A.chi + e.comp, e.hi);
}

__global__ __launch_bounds__(256) void mst_emit_kernel(const MstArgs A) {
  const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const EdgeKey e = edge_key(A, pos);
  if (!(e.act && e.wlo == A.cmin[e.comp] && e.hi == A.chi[e.comp])) return;
  const uint32_t n = (uint32_t)A.T.n;
  const uint32_t pos_p = A.best_pos[pos];
  if (pos_p >= n) {  // (never)
    atomicAdd(A.err, 1u);
    return;
  }
  const uint32_t d = A.comp[pos_p];
  if (d >= n) {  // (never: the candidate is a vertex)
    atomicAdd(A.err, 1u);
    return;
  }
  // the partner chose this edge too and has the smaller id: it writes and unites
  if (d < e.comp && A.cmin[d] == e.wlo && A.chi[d] == e.hi) return;
  const uint32_t slot = atomicAdd(A.count, 1u);
  if (slot >= n) {  // (never: a forest has fewer than n edges)
    atomicAdd(A.err, 1u);
    return;
  }
  A.erows[2 * (int64_t)slot] = (int32_t)(uint32_t)e.wlo;
  A.erows[2 * (int64_t)slot + 1] = (int32_t)e.hi;
  A.ew[slot] = lsk::bitsf((uint32_t)(e.wlo >> 32));
  uint32_t rq = (uint32_t)pos, retries = 0;
  bool bad = false;
  unite(A.parent, rq, pos_p, n, bad, retries);
  if (bad) atomicAdd(A.err, 1u);
  if (A.stats && retries) atomicAdd(&A.stats[4], (unsigned long long)retries);
}

// mst_labels: unite the two rows of every edge below the cutoff (strict, the predicate of
// radius.hip) in a forest over the rows themselves.
__global__ __launch_bounds__(256) void mst_cut_kernel(const int32_t *__restrict__ rows, const float *__restrict__ d2,
                                                      int64_t m, float cut2, uint32_t n, uint32_t *parent,
                                                      uint32_t *err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || !(d2[i] < cut2)) return;
  const uint32_t a = (uint32_t)rows[2 * i], b = (uint32_t)rows[2 * i + 1];
  if (a >= n || b >= n) {
    atomicAdd(err, 1u);
    return;
  }
  uint32_t rq = a, retries = 0;
  bool bad = false;
  unite(parent, rq, b, n, bad, retries);
  if (bad) atomicAdd(err, 1u);
}

}  // namespace

namespace {

// One round; period: null (open box) or three values > 0 (+inf: open axis).
int mst_round(const char *what, const lsk_tree_view *tree, const uint32_t *perm, const float *core,
              const float *period, uint32_t *parent, uint32_t *comp, uint32_t *ncomp, unsigned long long *best,
              uint32_t *best_pos, unsigned long long *cmin, uint32_t *chi, int32_t *erows, float *ew,
              uint32_t *count, uint32_t *err, unsigned long long *stats, void *stream) {
  if (!lsk_tree_ok(tree)) {
    lsk::set_last_error(std::string(what) + ": tree view incomplete (1 <= n < 2^31, depth = tree_depth(n))");
    return 1;
  }
  if (!perm || !parent || !comp || !ncomp || !best || !best_pos || !cmin || !chi || !erows || !ew || !count ||
      !err) {
    lsk::set_last_error(std::string(what) + ": null argument");
    return 1;
  }
  MstArgs A{};
  MstPeriod P{};
  for (int a = 0; period && a < 3; a++) {
    if (!(period[a] > 0.f)) {
      lsk::set_last_error(std::string(what) + ": period must be three values > 0 (+inf: open axis)");
      return 1;
    }
    P.L[a] = period[a];
  }
  A.T = *tree;
  A.perm = perm;
  A.core = core;
  A.parent = parent;
  A.comp = comp;
  A.ncomp = ncomp;
  A.best = best;
  A.best_pos = best_pos;
  A.cmin = cmin;
  A.chi = chi;
  A.erows = erows;
  A.ew = ew;
  A.count = count;
  A.err = err;
  A.stats = stats;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = A.T.n;
  const unsigned per_pos = lsk_blocks(n, 256);
  mst_comp_kernel<<<per_pos, 256, 0, st>>>(A);
  LSK_CHECK_LAUNCH("mst comp");
  mst_leaf_kernel<<<lsk_blocks((int64_t)1 << A.T.depth, kWaves), kWaves * 64, 0, st>>>(A);
  LSK_CHECK_LAUNCH("mst leaf");
  for (int level = A.T.depth - 1; level >= 0; level--) {
    mst_level_kernel<<<lsk_blocks((int64_t)1 << level, 256), 256, 0, st>>>(A, level);
    LSK_CHECK_LAUNCH("mst level");
  }
  const unsigned walk_blocks = lsk_blocks((n + lsk::kBucket - 1) / lsk::kBucket, kWaves);
  if (period) {
    if (core)
      mst_nearest_periodic_kernel<true><<<walk_blocks, kWaves * 64, 0, st>>>(A, P);
    else
      mst_nearest_periodic_kernel<false><<<walk_blocks, kWaves * 64, 0, st>>>(A, P);
  } else if (core) {
    mst_nearest_kernel<true><<<walk_blocks, kWaves * 64, 0, st>>>(A);
  } else {
    mst_nearest_kernel<false><<<walk_blocks, kWaves * 64, 0, st>>>(A);
  }
  LSK_CHECK_LAUNCH("mst nearest");
  mst_min1_kernel<<<per_pos, 256, 0, st>>>(A);
  LSK_CHECK_LAUNCH("mst min1");
  mst_min2_kernel<<<per_pos, 256, 0, st>>>(A);
  LSK_CHECK_LAUNCH("mst min2");
  mst_emit_kernel<<<per_pos, 256, 0, st>>>(A);
  LSK_CHECK_LAUNCH("mst emit");
  return 0;
}

}  // namespace

extern "C" int lsk_hip_mst_round(const lsk_tree_view *tree, const uint32_t *perm, const float *core,
                                 uint32_t *parent, uint32_t *comp, uint32_t *ncomp, unsigned long long *best,
                                 uint32_t *best_pos, unsigned long long *cmin, uint32_t *chi, int32_t *erows,
                                 float *ew, uint32_t *count, uint32_t *err, unsigned long long *stats,
                                 void *stream) {
  return mst_round("mst_round", tree, perm, core, nullptr, parent, comp, ncomp, best, best_pos, cmin, chi, erows, ew,
                   count, err, stats, stream);
}

extern "C" int lsk_hip_mst_periodic_round(const lsk_tree_view *tree, const uint32_t *perm, const float *core,
                                          const float *period, uint32_t *parent, uint32_t *comp, uint32_t *ncomp,
                                          unsigned long long *best, uint32_t *best_pos, unsigned long long *cmin,
                                          uint32_t *chi, int32_t *erows, float *ew, uint32_t *count, uint32_t *err,
                                          unsigned long long *stats, void *stream) {
  if (!period) {
    lsk::set_last_error("mst_periodic_round: period must be three values > 0 (+inf: open axis)");
    return 1;
  }
  return mst_round("mst_periodic_round", tree, perm, core, period, parent, comp, ncomp, best, best_pos, cmin, chi,
                   erows, ew, count, err, stats, stream);
}

extern "C" int lsk_hip_mst_cut(const int32_t *rows, const float *d2, int64_t m, float cut2, int64_t n,
                               uint32_t *parent, uint32_t *err, void *stream) {
  if (m < 0 || n < 1 || n >= ((int64_t)1 << 31) || !(cut2 >= 0.f)) {
    lsk::set_last_error("mst_cut: m >= 0, 1 <= n < 2^31 and cut2 >= 0 required");
    return 1;
  }
  if (!parent || !err || (m > 0 && (!rows || !d2))) {
    lsk::set_last_error("mst_cut: null argument");
    return 1;
  }
  if (m == 0) return 0;
  mst_cut_kernel<<<lsk_blocks(m, 256), 256, 0, (hipStream_t)stream>>>(rows, d2, m, cut2, (uint32_t)n, parent, err);
  LSK_CHECK_LAUNCH("mst cut");
  return 0;
}
