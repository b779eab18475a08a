// lsknn host library — C ABI (loaded from Python with ctypes; usable from C++ apps).
//
// Components (SURVEY §2 IDs):
//   A01/A02/A03  CLI grammar of both reference entrypoints        -> lsk_cli_parse
//   A06          readFilePortion<float3> partition semantics       -> lsk_io_portion / lsk_io_read
//   A07          readListOfFileNames (fixed: CRLF, no trailing \n)  -> lsk_io_read_filelist
//   A22/A23      output writers (parallel pwrite, same bytes)      -> lsk_io_write
//   A18-A21      prePartitioned peer schedule                      -> lsk_peer_*
//   T1 oracle    exact CPU k-th-distance (brute force / k-d tree)  -> lsk_cpu_kth_*
//   CPU backend  Morton keys, bounds, halo filter for gloo tests   -> lsk_cpu_*
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// ---------------------------------------------------------------- version / info
int lsk_host_abi_version(void);

// ---------------------------------------------------------------- CLI (A01-A03, C7)
// variant: 0 = unorderedData, 1 = prePartitionedData.
// Returns 0 on success; otherwise the exit code usage() would use (1) and writes the
// complete stderr text the reference prints into `err` (NUL-terminated, truncated to
// errlen). Extension flags (all long options, defaults never change reference
// behaviour) are parsed into the same struct.
typedef struct lsk_cli_args {
  char input[4096];   // positional (last wins)
  char output[4096];  // -o
  int k;              // -k
  float max_radius;   // -r  (default +inf)
  int gpu_affinity;   // -g  (0 = unset)
  // extensions
  char mode[32];      // --mode {auto,halo,ring,peer}
  char device[16];    // --device {auto,cuda,cpu}
  char stats[4096];   // --stats <file.json>
  int verbose;        // -v / --verbose
  char bootstrap[16]; // --bootstrap {auto,env,mpi,spawn}: where rank/size come from
  int nproc;          // --nproc N: ranks started by --bootstrap spawn (0 = unset)
  char device_map[256];  // --device-map 0,1,...: local rank i uses GPU map[i % len]
  char balance[8];    // --balance {auto,on,off}: prePartitioned load rebalancing
} lsk_cli_args;

int lsk_cli_parse(int variant, int argc, const char **argv, lsk_cli_args *out, char *err,
                  int errlen);

// ---------------------------------------------------------------- I/O (A06, A07, A22/A23)
// Reference partition: numData = bytes/recsize, rank r of P gets
// [floor(numData*r/P), floor(numData*(r+1)/P)). Returns 0 or -errno.
int lsk_io_portion(const char *path, int64_t rank, int64_t size, int64_t recsize,
                   int64_t *begin, int64_t *count, int64_t *total);
// Multi-threaded pread of nbytes at offset into dst. Returns 0 or -errno.
int lsk_io_read(const char *path, int64_t offset, int64_t nbytes, void *dst, int nthreads);
// Multi-threaded pwrite. flags bit0: create+truncate first, bit1: ftruncate to
// `total_size` (when >= 0) before writing. Returns 0 or -errno.
int lsk_io_write(const char *path, int64_t offset, const void *src, int64_t nbytes,
                 int flags, int64_t total_size, int nthreads);
// Reads a file list. Writes names separated by '\n' into buf; returns the number of
// names, or -errno, or -(needed bytes) - 1000000 if buf is too small.
int64_t lsk_io_read_filelist(const char *path, char *buf, int64_t buflen);

// ---------------------------------------------------------------- peer schedule (A18-A21)
// Sattolo permutation seeded exactly like the reference (srand(rank+0x1234567), 10
// discarded rand() calls). Writes `size` ints.
void lsk_peer_permutation(int rank, int size, int *out);
// boxes: 6 floats per rank (lo.xyz, hi.xyz). seen: one byte per rank. Returns the
// requested peer or -1 (strictly closest by box gap among unseen peers with gap <
// cutoff; ties go to the first in permutation order).
int lsk_peer_choose(const float *my_box, const float *all_boxes, int size, float cutoff,
                    const uint8_t *seen, const int *perm);
float lsk_box_distance(const float *a, const float *b);

// ---------------------------------------------------------------- CPU oracle (T1)
// Result semantics: for every query, the k-th smallest of the multiset
// { dist2(q,p) : p in points, dist2 < cut2 } ∪ { cut2 repeated k }, as a squared
// distance. cut2 = r*r (float) or +inf.
void lsk_cpu_kth_brute(const float *pts, int64_t n, const float *qry, int64_t nq, int k,
                       float cut2, float *out_d2, int nthreads);
// Neighbour lists by brute force: per query the first k of { (dist2, i) : dist2 < cut2 } in
// ascending (dist2 bits, input row i) order -> out_idx / out_d2 [nq][k]; unfilled slots get
// -1 / cut2. out_d2[q][k-1] is what lsk_cpu_kth_brute returns.
void lsk_cpu_knn_brute(const float *pts, int64_t n, const float *qry, int64_t nq, int k,
                       float cut2, int32_t *out_idx, float *out_d2, int nthreads);
// Fixed-radius search by brute force: counts[q] = #{ i : dist2(q, p_i) < cut2 } (strict; a
// query with a NaN or infinite coordinate counts nothing), and the rows themselves in CSR
// form: row q = [offsets[q], offsets[q+1]) (offsets: the exclusive prefix sum of the counts
// for the same cut2, nq + 1 entries) receives every such (input row i, dist2) in ascending
// (dist2 bits, i) order.
void lsk_cpu_radius_count(const float *pts, int64_t n, const float *qry, int64_t nq, float cut2,
                          int32_t *counts, int nthreads);
void lsk_cpu_radius_fill(const float *pts, int64_t n, const float *qry, int64_t nq, float cut2,
                         const int64_t *offsets, int32_t *out_idx, float *out_d2, int nthreads);
// The same with a squared cutoff per query (qcut2 [nq], optional) and / or per point (pcut2
// [n], optional): point i is in row q iff dist2 < qcut2[q] (when given) and dist2 < pcut2[i]
// (when given). Same CSR form and row order.
void lsk_cpu_radius_var_count(const float *pts, int64_t n, const float *qry, int64_t nq, const float *qcut2,
                              const float *pcut2, int32_t *counts, int nthreads);
void lsk_cpu_radius_var_fill(const float *pts, int64_t n, const float *qry, int64_t nq, const float *qcut2,
                             const float *pcut2, const int64_t *offsets, int32_t *out_idx, float *out_d2,
                             int nthreads);
// Density clustering (friends-of-friends / DBSCAN) by brute force over all pairs. core[i] = 1
// iff #{ j : dist2(p_i, p_j) < cut2 } >= min_pts (strict; the point itself and exact copies
// count; a point with a NaN or infinite coordinate counts nothing). labels[i]: a core point
// gets the smallest row among the core points of its connected component (edges: pairs of
// core points with dist2 < cut2); a non-core point the label of the core point smallest by
// (dist2 bits, row) among those with dist2 < cut2, and without one -1, or i when min_pts = 1.
void lsk_cpu_cluster(const float *pts, int64_t n, float cut2, int min_pts, int32_t *labels, uint8_t *core,
                     int nthreads);
// Euclidean minimum spanning tree by brute force (Prim over all pairs). Vertices: the points with
// finite coordinates. Weight of {a, b}: w = dist2, or with core (optional, [n] floats >= 0)
// max(dist2, core[a], core[b]). Edges are ordered by (bits of w, lo, hi), lo < hi the rows: a
// strict total order, so the tree is unique. rows (int32 [m][2], (lo, hi)) and d2 ([m], w) receive
// the m = max(finite points - 1, 0) edges ascending by that key (room for n - 1); returns m.
int64_t lsk_cpu_mst(const float *pts, int64_t n, const float *core, int32_t *rows, float *d2);
// lsk_cpu_mst under a period (three values > 0, +inf = open axis): dist2 is replaced by the
// minimum image of the difference (below), whatever the length of an edge.
int64_t lsk_cpu_mst_periodic(const float *pts, int64_t n, const float *core, const float *period, int32_t *rows,
                             float *d2);
// labels[i] (int32 [n]) = the smallest row of i's component under the edges with d2 < cut2
// (strict); returns non-zero when an edge names a row outside [0, n).
int lsk_cpu_mst_labels(const int32_t *rows, const float *d2, int64_t m, float cut2, int64_t n, int32_t *labels);
// The radius search and the clustering above under a period (three values > 0, +inf = open axis): dist2 is replaced by the
// minimum image of the difference — per axis d = q - p, h = 0.5f * L, d > h: d - L, d < -h:
// d + L, in float32 and in this order — then the canonical dist2. qcut2 (optional, [nq])
// replaces cut2 per query.
void lsk_cpu_radius_periodic_count(const float *pts, int64_t n, const float *qry, int64_t nq, float cut2,
                                   const float *qcut2, const float *period, int32_t *counts, int nthreads);
void lsk_cpu_radius_periodic_fill(const float *pts, int64_t n, const float *qry, int64_t nq, float cut2,
                                  const float *qcut2, const float *period, const int64_t *offsets,
                                  int32_t *out_idx, float *out_d2, int nthreads);
void lsk_cpu_cluster_periodic(const float *pts, int64_t n, float cut2, int min_pts, const float *period,
                              int32_t *labels, uint8_t *core, int nthreads);
// The radius search with a squared cutoff on both sides (qcut2 [nq], pcut2 [n], both given):
// point i is in row q iff d² < max(qcut2[q], pcut2[i]) (rule = 0, either) or d² < min(qcut2[q],
// pcut2[i]) (rule = 1, both), strictly; d² = dist2, or with period (optional, as above) the
// minimum image. Same CSR form and row order.
void lsk_cpu_radius_reach_count(const float *pts, int64_t n, const float *qry, int64_t nq, const float *qcut2,
                                const float *pcut2, int rule, const float *period, int32_t *counts, int nthreads);
void lsk_cpu_radius_reach_fill(const float *pts, int64_t n, const float *qry, int64_t nq, const float *qcut2,
                               const float *pcut2, int rule, const float *period, const int64_t *offsets,
                               int32_t *out_idx, float *out_d2, int nthreads);
// Radius profile by brute force, one pass over the points per query: out[q * nb + b] (int32 [nq,
// nb]) = #{ i : dist2(q, p_i) < cut2s[b] } for nb >= 1 ascending cutoffs (each >= 0, +inf
// allowed, no NaN), i.e. column b is lsk_cpu_radius_count at cut2s[b]; period (optional, as
// above): lsk_cpu_radius_periodic_count at cut2s[b].
void lsk_cpu_radius_profile(const float *pts, int64_t n, const float *qry, int64_t nq, const float *cut2s,
                            int32_t nb, const float *period, int32_t *out, int nthreads);
// The same with a weight per point: out[q * nb + b] (int64 [nq, nb]) = the sum of w[i] (int64 [n],
// negative allowed) over { i : dist2(q, p_i) < cut2s[b] }; with every weight 1 the counts above.
// Sums wrap in 64 bits: exact when sum |w| < 2^63.
void lsk_cpu_weighted_profile(const float *pts, int64_t n, const float *qry, int64_t nq, const float *cut2s,
                              int32_t nb, const float *period, const int64_t *w, int64_t *out, int nthreads);
// Anisotropic pair counts and weighted pair sums by brute force over all pairs: out (int64 [na, nb])
// is cumulative on both axes. los in {0, 1, 2} picks the line-of-sight difference dl of q - p
// (period: its minimum image); par2 = dl * dl, perp2 = fmaf(db, db, da * da) of the other two axes
// in ascending order. mode 0: out[i, j] = #{pairs : perp2 < a2[i] and par2 < b2[j]}; mode 1: #{pairs
// : d2 < a2[i] and par2 < b2[j] * d2}. a2 / b2: na, nb >= 1 ascending values >= 0, +inf allowed, no
// NaN. What is null:
//  * period: the open box.
//  * w (int64 [n]): counts, every pair adds 1. Else wq[q] * w[i] is added per pair (wq: int64 [nq] or
//    null = all ones; negative allowed; wq without w is ignored). Sums and products wrap in 64 bits:
//    exact when (sum |w|) * (sum |wq|) < 2^63. With unit weights the counts.
//  * observer: the axis los. Else (open box: period null, los unused) the line of sight of an
//    observer (three finite floats): per pair l = (q - o) + (p - o) per axis (twice observer ->
//    midpoint), sl = fmaf(dz, lz, fmaf(dy, ly, dx * lx)), ll = dist2(l), par2 = (sl / ll) * sl, perp2
//    = d2 - par2, a negative perp2 becoming 0 and a NaN staying one; the same cells. A pair whose
//    midpoint is the observer (ll == 0) counts nowhere.
void lsk_cpu_pair_sums_2d(const float *pts, int64_t n, const float *qry, int64_t nq, const float *a2, int32_t na,
                          const float *b2, int32_t nb, int mode, int los, const float *period,
                          const float *observer, const int64_t *w, const int64_t *wq, int64_t *out, int nthreads);
// lsk_cpu_kth_brute / lsk_cpu_knn_brute under a period: brute force over all points with the
// periodic squared distance above, the same selection (k-th smallest by bits among those <
// cut2, else cut2) and the same tie rule (ascending (d² bits, row); unfilled: -1 / cut2).
void lsk_cpu_kth_periodic(const float *pts, int64_t n, const float *qry, int64_t nq, int k, float cut2,
                          const float *period, float *out_d2, int nthreads);
void lsk_cpu_knn_periodic(const float *pts, int64_t n, const float *qry, int64_t nq, int k, float cut2,
                          const float *period, int32_t *out_idx, float *out_d2, int nthreads);
// Verification counts (= lsk_hip_count_below): counts[2j] +=#{p : dist2(q_j,p) < thr[2j]},
// counts[2j+1] += #{p : dist2(q_j,p) < thr[2j+1]}.
void lsk_cpu_count_below(const float *pts, int64_t n, const float *qry, const float *thr, int nq,
                         unsigned long long *counts, int nthreads);
// Same result via a CPU k-d tree (object-median, leaf buckets) built over `pts`.
void lsk_cpu_kth_kdtree(const float *pts, int64_t n, const float *qry, int64_t nq, int k,
                        float cut2, float *out_d2, int nthreads);

// ---------------------------------------------------------------- CPU backend ops
// AABB of n points -> box[6]. Empty set -> (+inf,-inf).
void lsk_cpu_bounds(const float *pts, int64_t n, float *box, int nthreads);
// 30-bit curve keys (curve: 0 = Morton, 1 = Hilbert) relative to a cube (origin,
// scale = 1024/extent).
void lsk_cpu_morton(const float *pts, int64_t n, const float *origin, float scale,
                    uint32_t *keys, int curve, int nthreads);
// For each point, the bitmask (bit j) of target sets it must be sent to: point p goes
// to set j iff box_dist2(p, box) < r2 for some box of set j. boxes: 8 floats each
// (lo.xyz, r2, hi.xyz, pad); box_offsets: nsets+1 offsets. skip_set excluded (-1 none).
void lsk_cpu_halo_mask(const float *pts, int64_t n, const float *boxes,
                       const int64_t *box_offsets, int nsets, int skip_set,
                       uint64_t *mask, int nthreads);

// ---------------------------------------------------------------- ref-algo (CPU twin)
// Left-balanced k-d tree (object median, round-robin axis): out_pts in tree order,
// out_ids[i] = input index of tree node i (may be NULL).
void lsk_cpu_lbt_build(const float *pts, int64_t n, float *out_pts, uint32_t *out_ids);
// Stack-free traversal + persisted k-max-heaps (AoS [nq][k] of d2bits<<32|id); init=1
// (re)initialises with cut2; rmax (optional) receives max(rmax, max_q sqrt(top_q)).
void lsk_cpu_refalgo_knn(const float *tree, int64_t n, const float *qpts, int64_t nq,
                         unsigned long long *heaps, int k, float cut2, int init, float *rmax,
                         uint32_t id_base, int nthreads);
void lsk_cpu_refalgo_extract(const unsigned long long *heaps, int64_t nq, int k, float *out);

#ifdef __cplusplus
}
#endif
