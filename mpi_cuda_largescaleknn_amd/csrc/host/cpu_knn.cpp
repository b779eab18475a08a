// CPU exact k-th-distance oracle + CPU backend ops (bounds, Morton, halo mask).
//
// The oracle defines the result the GPU must reproduce bit-for-bit:
// out[q] = k-th smallest of { dist2(q,p) < cut2 } ∪ { cut2 × k }, which is exactly what
// the reference's FlexHeapCandidateList (initialised with cutOff², strict '<' push;
// unorderedDataVariant.cu:84-86, 97-98) leaves on top of its heap.
#include "lsk_host.h"
#include "../common.h"

#include <algorithm>
#include <array>
#include <mutex>
#include <atomic>
#include <cmath>
#include <limits>
#include <thread>
#include <vector>

using lsk::vec3f;

namespace {

template <typename F>
void parallel_for(int64_t n, int nthreads, F &&fn) {
  if (n <= 0) return;
  if (nthreads < 1) nthreads = 1;
  int64_t nt = std::min<int64_t>(nthreads, n);
  if (nt == 1) {
    fn(0, n);
    return;
  }
  // Dynamic chunking: query costs vary a lot with local density.
  std::atomic<int64_t> next{0};
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(4096, n / (nt * 16) + 1));
  std::vector<std::thread> th;
  for (int64_t t = 0; t < nt; t++) {
    th.emplace_back([&] {
      for (;;) {
        int64_t b = next.fetch_add(chunk);
        if (b >= n) break;
        fn(b, std::min(n, b + chunk));
      }
    });
  }
  for (auto &x : th) x.join();
}

// k-max-heap over squared distances, initialised with k copies of cut2.
struct KHeap {
  std::vector<float> h;
  void reset(int k, float cut2) { h.assign((size_t)k, cut2); }
  float top() const { return h[0]; }
  void push(float v) {  // precondition: v < top()
    const int n = (int)h.size();
    int i = 0;
    for (;;) {
      int l = 2 * i + 1, r = l + 1, c = i;
      float cv = v;
      if (l < n && h[l] > cv) { c = l; cv = h[l]; }
      if (r < n && h[r] > cv) { c = r; cv = h[r]; }
      if (c == i) break;
      h[i] = h[c];
      i = c;
    }
    h[i] = v;
  }
};

struct KdNode {
  float lo[3], hi[3];
  int64_t begin, end;   // point range (leaf) or children
  int64_t left, right;  // -1 for leaf
};

struct KdTree {
  std::vector<vec3f> pts;
  std::vector<KdNode> nodes;
  static constexpr int kLeaf = 16;

  int64_t build(int64_t b, int64_t e) {
    KdNode nd;
    for (int a = 0; a < 3; a++) {
      nd.lo[a] = std::numeric_limits<float>::infinity();
      nd.hi[a] = -std::numeric_limits<float>::infinity();
    }
    for (int64_t i = b; i < e; i++) {
      const float c[3] = {pts[i].x, pts[i].y, pts[i].z};
      for (int a = 0; a < 3; a++) {
        nd.lo[a] = std::min(nd.lo[a], c[a]);
        nd.hi[a] = std::max(nd.hi[a], c[a]);
      }
    }
    nd.begin = b;
    nd.end = e;
    nd.left = nd.right = -1;
    int64_t id = (int64_t)nodes.size();
    nodes.push_back(nd);
    if (e - b > kLeaf) {
      int axis = 0;
      float w = nd.hi[0] - nd.lo[0];
      for (int a = 1; a < 3; a++)
        if (nd.hi[a] - nd.lo[a] > w) { w = nd.hi[a] - nd.lo[a]; axis = a; }
      int64_t m = (b + e) / 2;
      std::nth_element(pts.begin() + b, pts.begin() + m, pts.begin() + e,
                       [axis](const vec3f &p, const vec3f &q) {
                         return (&p.x)[axis] < (&q.x)[axis];
                       });
      int64_t l = build(b, m);
      int64_t r = build(m, e);
      nodes[id].left = l;
      nodes[id].right = r;
    }
    return id;
  }

  float node_dist2(const KdNode &n, const vec3f &q) const {
    return lsk::box_dist2(q, vec3f{n.lo[0], n.lo[1], n.lo[2]}, vec3f{n.hi[0], n.hi[1], n.hi[2]});
  }

  float query(const vec3f &q, int k, float cut2, KHeap &heap,
              std::vector<std::pair<int64_t, float>> &stack) const {
    heap.reset(k, cut2);
    if (nodes.empty()) return heap.top();
    stack.clear();
    stack.push_back({0, node_dist2(nodes[0], q)});
    while (!stack.empty()) {
      auto [ni, bd] = stack.back();
      stack.pop_back();
      if (!(bd < heap.top())) continue;
      const KdNode &n = nodes[ni];
      if (n.left < 0) {
        for (int64_t i = n.begin; i < n.end; i++) {
          float d2 = lsk::dist2(q, pts[i]);
          if (d2 < heap.top()) heap.push(d2);
        }
        continue;
      }
      float dl = node_dist2(nodes[n.left], q), dr = node_dist2(nodes[n.right], q);
      if (dl <= dr) {
        stack.push_back({n.right, dr});
        stack.push_back({n.left, dl});
      } else {
        stack.push_back({n.left, dl});
        stack.push_back({n.right, dr});
      }
    }
    return heap.top();
  }
};

}  // namespace

extern "C" void lsk_cpu_kth_brute(const float *pts, int64_t n, const float *qry, int64_t nq,
                                  int k, float cut2, float *out_d2, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<float> d;
    d.reserve((size_t)n);
    for (int64_t qi = b; qi < e; qi++) {
      d.clear();
      for (int64_t i = 0; i < n; i++) {
        float v = lsk::dist2(Q[qi], P[i]);
        if (v < cut2) d.push_back(v);
      }
      if ((int64_t)d.size() < k) {
        out_d2[qi] = cut2;
      } else {
        std::nth_element(d.begin(), d.begin() + (k - 1), d.end());
        out_d2[qi] = d[(size_t)k - 1];
      }
    }
  });
}

extern "C" void lsk_cpu_knn_brute(const float *pts, int64_t n, const float *qry, int64_t nq,
                                  int k, float cut2, int32_t *out_idx, float *out_d2, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<uint64_t> d;  // d2 bits << 32 | input row (non-negative floats order like their bits)
    d.reserve((size_t)n);
    for (int64_t qi = b; qi < e; qi++) {
      d.clear();
      for (int64_t i = 0; i < n; i++) {
        const float v = lsk::dist2(Q[qi], P[i]);
        if (v < cut2) d.push_back(((uint64_t)lsk::fbits(v) << 32) | (uint32_t)i);
      }
      const size_t m = std::min<size_t>(d.size(), (size_t)k);
      std::partial_sort(d.begin(), d.begin() + m, d.end());
      for (size_t j = 0; j < (size_t)k; j++) {
        out_idx[qi * k + (int64_t)j] = j < m ? (int32_t)(uint32_t)d[j] : -1;
        out_d2[qi * k + (int64_t)j] = j < m ? lsk::bitsf((uint32_t)(d[j] >> 32)) : cut2;
      }
    }
  });
}

extern "C" void lsk_cpu_radius_count(const float *pts, int64_t n, const float *qry, int64_t nq, float cut2,
                                     int32_t *counts, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t qi = b; qi < e; qi++) {
      int32_t c = 0;
      for (int64_t i = 0; i < n; i++) c += lsk::dist2(Q[qi], P[i]) < cut2;
      counts[qi] = c;
    }
  });
}

extern "C" void lsk_cpu_radius_fill(const float *pts, int64_t n, const float *qry, int64_t nq, float cut2,
                                    const int64_t *offsets, int32_t *out_idx, float *out_d2, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<uint64_t> d;  // d2 bits << 32 | input row, as lsk_cpu_knn_brute
    for (int64_t qi = b; qi < e; qi++) {
      d.clear();
      for (int64_t i = 0; i < n; i++) {
        const float v = lsk::dist2(Q[qi], P[i]);
        if (v < cut2) d.push_back(((uint64_t)lsk::fbits(v) << 32) | (uint32_t)i);
      }
      std::sort(d.begin(), d.end());
      // (offsets come from lsk_cpu_radius_count with the same cut2: the row holds d.size() slots)
      const size_t m = std::min<size_t>(d.size(), (size_t)(offsets[qi + 1] - offsets[qi]));
      for (size_t j = 0; j < m; j++) {
        out_idx[offsets[qi] + (int64_t)j] = (int32_t)(uint32_t)d[j];
        out_d2[offsets[qi] + (int64_t)j] = lsk::bitsf((uint32_t)(d[j] >> 32));
      }
    }
  });
}

// Variable radii: point i is in row q iff d² < qcut2[q] (when given) and d² < pcut2[i] (when
// given).
extern "C" void lsk_cpu_radius_var_count(const float *pts, int64_t n, const float *qry, int64_t nq,
                                         const float *qcut2, const float *pcut2, int32_t *counts, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t qi = b; qi < e; qi++) {
      int32_t c = 0;
      for (int64_t i = 0; i < n; i++) {
        const float v = lsk::dist2(Q[qi], P[i]);
        c += (!qcut2 || v < qcut2[qi]) && (!pcut2 || v < pcut2[i]);
      }
      counts[qi] = c;
    }
  });
}

extern "C" void lsk_cpu_radius_var_fill(const float *pts, int64_t n, const float *qry, int64_t nq,
                                        const float *qcut2, const float *pcut2, const int64_t *offsets,
                                        int32_t *out_idx, float *out_d2, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<uint64_t> d;  // d2 bits << 32 | input row, as lsk_cpu_knn_brute
    for (int64_t qi = b; qi < e; qi++) {
      d.clear();
      for (int64_t i = 0; i < n; i++) {
        const float v = lsk::dist2(Q[qi], P[i]);
        if ((!qcut2 || v < qcut2[qi]) && (!pcut2 || v < pcut2[i]))
          d.push_back(((uint64_t)lsk::fbits(v) << 32) | (uint32_t)i);
      }
      std::sort(d.begin(), d.end());
      // (offsets come from lsk_cpu_radius_var_count with the same cutoffs)
      const size_t m = std::min<size_t>(d.size(), (size_t)(offsets[qi + 1] - offsets[qi]));
      for (size_t j = 0; j < m; j++) {
        out_idx[offsets[qi] + (int64_t)j] = (int32_t)(uint32_t)d[j];
        out_d2[offsets[qi] + (int64_t)j] = lsk::bitsf((uint32_t)(d[j] >> 32));
      }
    }
  });
}

// Density clustering by brute force, the definition itself: core[i] = #{ j : dist2 < cut2 } >=
// min_pts; clusters = connected components of the core points under dist2 < cut2, labelled
// with their smallest row (the union-find hooks the larger root under the smaller, so a root
// is its component's smallest row); a non-core point takes the label of its nearest core
// point by (dist2 bits, row), or -1 (min_pts = 1: its own row) when it has none. The counts
// and the border points are threaded; the unions run over all pairs in one thread.
extern "C" void lsk_cpu_cluster(const float *pts, int64_t n, float cut2, int min_pts, int32_t *labels,
                                uint8_t *core, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  parallel_for(n, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t i = b; i < e; i++) {
      int64_t c = 0;
      for (int64_t j = 0; j < n; j++) c += lsk::dist2(P[i], P[j]) < cut2;
      core[i] = c >= (int64_t)min_pts;
    }
  });
  std::vector<int32_t> parent((size_t)n);
  for (int64_t i = 0; i < n; i++) parent[(size_t)i] = (int32_t)i;
  auto find = [&](int32_t x) {
    while (parent[(size_t)x] != x) {
      parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
      x = parent[(size_t)x];
    }
    return x;
  };
  for (int64_t i = 0; i < n; i++) {
    if (!core[i]) continue;
    for (int64_t j = i + 1; j < n; j++) {
      if (!core[j] || !(lsk::dist2(P[i], P[j]) < cut2)) continue;
      const int32_t a = find((int32_t)i), c = find((int32_t)j);
      if (a != c) parent[(size_t)std::max(a, c)] = std::min(a, c);
    }
  }
  for (int64_t i = 0; i < n; i++)
    if (core[i]) labels[i] = find((int32_t)i);
  // (the roots are final: the border points only read them)
  parallel_for(n, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t i = b; i < e; i++) {
      if (core[i]) continue;
      uint64_t best = ~0ull;
      for (int64_t j = 0; j < n; j++) {
        if (!core[j]) continue;
        const float v = lsk::dist2(P[i], P[j]);
        if (v < cut2) best = std::min(best, ((uint64_t)lsk::fbits(v) << 32) | (uint32_t)j);
      }
      if (best != ~0ull)
        labels[i] = labels[(size_t)(uint32_t)best];
      else
        labels[i] = min_pts == 1 ? (int32_t)i : -1;
    }
  });
}

// Euclidean minimum spanning tree by brute force: Prim over all pairs of finite points under the
// strict total order (bits of w, lo, hi), O(n²) time and O(n) memory. The order being total,
// the MST is unique: any correct algorithm yields this edge set. Edges come out sorted by key.
// pair(p, q): the squared distance of two points (open box: dist2; periodic: the minimum image).
namespace {

template <class Pair>
int64_t mst_prim(const float *pts, int64_t n, const float *core, int32_t *rows, float *d2, Pair pair) {
  const vec3f *P = (const vec3f *)pts;
  struct Key {
    uint64_t wlo;  // bits of w << 32 | lo
    uint32_t hi;
    bool operator<(const Key &o) const { return wlo != o.wlo ? wlo < o.wlo : hi < o.hi; }
  };
  std::vector<int32_t> v;  // the vertices outside the tree
  for (int64_t i = 0; i < n; i++)
    if (std::isfinite(P[i].x) && std::isfinite(P[i].y) && std::isfinite(P[i].z)) v.push_back((int32_t)i);
  if (v.size() < 2) return 0;
  auto key = [&](int32_t a, int32_t b) {
    float w = pair(P[a], P[b]);
    if (core) w = std::max(std::max(w, core[a] + 0.f), core[b] + 0.f);  // (+ 0.f: -0 has other bits)
    return Key{((uint64_t)lsk::fbits(w) << 32) | (uint32_t)std::min(a, b), (uint32_t)std::max(a, b)};
  };
  std::vector<Key> best(v.size(), Key{~0ull, ~0u});  // beside v: the smallest edge into the tree
  std::vector<Key> out;
  int32_t last = v[0];  // the vertex that joined the tree last
  v[0] = v.back();
  v.pop_back();
  best.pop_back();
  while (!v.empty()) {
    size_t arg = 0;
    for (size_t i = 0; i < v.size(); i++) {
      const Key k = key(v[i], last);
      if (k < best[i]) best[i] = k;
      if (best[i] < best[arg]) arg = i;
    }
    out.push_back(best[arg]);
    last = v[arg];
    v[arg] = v.back();
    best[arg] = best.back();
    v.pop_back();
    best.pop_back();
  }
  std::sort(out.begin(), out.end());
  for (size_t i = 0; i < out.size(); i++) {
    rows[2 * i] = (int32_t)(uint32_t)out[i].wlo;
    rows[2 * i + 1] = (int32_t)out[i].hi;
    d2[i] = lsk::bitsf((uint32_t)(out[i].wlo >> 32));
  }
  return (int64_t)out.size();
}

}  // namespace

extern "C" int64_t lsk_cpu_mst(const float *pts, int64_t n, const float *core, int32_t *rows, float *d2) {
  return mst_prim(pts, n, core, rows, d2, [](const vec3f &a, const vec3f &b) { return lsk::dist2(a, b); });
}

// The components of the edges with d2 < cut2 (strict) over rows 0 .. n - 1, each labelled by its
// smallest row: the host form of mst_labels.
extern "C" int lsk_cpu_mst_labels(const int32_t *rows, const float *d2, int64_t m, float cut2, int64_t n,
                                  int32_t *labels) {
  for (int64_t i = 0; i < n; i++) labels[i] = (int32_t)i;
  auto find = [&](int32_t x) {
    while (labels[x] != x) {
      labels[x] = labels[labels[x]];
      x = labels[x];
    }
    return x;
  };
  for (int64_t i = 0; i < m; i++) {
    if (!(d2[i] < cut2)) continue;
    const int64_t a0 = rows[2 * i], b0 = rows[2 * i + 1];
    if (a0 < 0 || b0 < 0 || a0 >= n || b0 >= n) return 1;
    const int32_t a = find((int32_t)a0), b = find((int32_t)b0);
    if (a != b) labels[std::max(a, b)] = std::min(a, b);
  }
  for (int64_t i = 0; i < n; i++) labels[i] = find((int32_t)i);
  return 0;
}

// ---- periodic box: the minimum image of the difference, written out literally ----------------
// Per axis d = q - p; h = 0.5f * L; d > h: d - L; d < -h: d + L (L = inf never wraps); then the
// canonical dist2. Symmetric in its bits (fl(q - p) = -fl(p - q), mirrored branches).
namespace {

inline float wrap_diff(float d, float L) {
  const float h = 0.5f * L;
  if (d > h)
    d = d - L;
  else if (d < -h)
    d = d + L;
  return d;
}

inline float pdist2(const vec3f &q, const vec3f &p, const float *L) {
  return lsk::dist2(wrap_diff(q.x - p.x, L[0]), wrap_diff(q.y - p.y, L[1]), wrap_diff(q.z - p.z, L[2]));
}

}  // namespace

// lsk_cpu_mst with the pair weight pd2 (symmetric in its bits, so the weight of a pair is well
// defined); no bound on an edge's length.
extern "C" int64_t lsk_cpu_mst_periodic(const float *pts, int64_t n, const float *core, const float *period,
                                        int32_t *rows, float *d2) {
  return mst_prim(pts, n, core, rows, d2, [=](const vec3f &a, const vec3f &b) { return pdist2(a, b, period); });
}

// lsk_cpu_radius_count under a period; qcut2 (optional, [nq]) replaces cut2 per query.
extern "C" void lsk_cpu_radius_periodic_count(const float *pts, int64_t n, const float *qry, int64_t nq, float cut2,
                                              const float *qcut2, const float *period, int32_t *counts,
                                              int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t qi = b; qi < e; qi++) {
      const float c2 = qcut2 ? qcut2[qi] : cut2;
      int32_t c = 0;
      for (int64_t i = 0; i < n; i++) c += pdist2(Q[qi], P[i], period) < c2;
      counts[qi] = c;
    }
  });
}

// lsk_cpu_radius_fill under a period, the same CSR form and row order.
extern "C" void lsk_cpu_radius_periodic_fill(const float *pts, int64_t n, const float *qry, int64_t nq, float cut2,
                                             const float *qcut2, const float *period, const int64_t *offsets,
                                             int32_t *out_idx, float *out_d2, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<uint64_t> d;  // d2 bits << 32 | input row, as lsk_cpu_knn_brute
    for (int64_t qi = b; qi < e; qi++) {
      const float c2 = qcut2 ? qcut2[qi] : cut2;
      d.clear();
      for (int64_t i = 0; i < n; i++) {
        const float v = pdist2(Q[qi], P[i], period);
        if (v < c2) d.push_back(((uint64_t)lsk::fbits(v) << 32) | (uint32_t)i);
      }
      std::sort(d.begin(), d.end());
      // (offsets come from lsk_cpu_radius_periodic_count with the same cutoffs)
      const size_t m = std::min<size_t>(d.size(), (size_t)(offsets[qi + 1] - offsets[qi]));
      for (size_t j = 0; j < m; j++) {
        out_idx[offsets[qi] + (int64_t)j] = (int32_t)(uint32_t)d[j];
        out_d2[offsets[qi] + (int64_t)j] = lsk::bitsf((uint32_t)(d[j] >> 32));
      }
    }
  });
}

// Two-sided radii: point i is in row q iff d² < max(qcut2[q], pcut2[i]) (rule 0, either) or d² <
// min(qcut2[q], pcut2[i]) (rule 1, both); d² = dist2, or pdist2 under a period (optional).
namespace {

inline float reach_cut(float cq, float cp, int rule) { return rule ? std::min(cq, cp) : std::max(cq, cp); }

inline float reach_d2(const vec3f &q, const vec3f &p, const float *period) {
  return period ? pdist2(q, p, period) : lsk::dist2(q, p);
}

}  // namespace

extern "C" void lsk_cpu_radius_reach_count(const float *pts, int64_t n, const float *qry, int64_t nq,
                                           const float *qcut2, const float *pcut2, int rule, const float *period,
                                           int32_t *counts, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t qi = b; qi < e; qi++) {
      int32_t c = 0;
      for (int64_t i = 0; i < n; i++) c += reach_d2(Q[qi], P[i], period) < reach_cut(qcut2[qi], pcut2[i], rule);
      counts[qi] = c;
    }
  });
}

extern "C" void lsk_cpu_radius_reach_fill(const float *pts, int64_t n, const float *qry, int64_t nq,
                                          const float *qcut2, const float *pcut2, int rule, const float *period,
                                          const int64_t *offsets, int32_t *out_idx, float *out_d2, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<uint64_t> d;  // d2 bits << 32 | input row, as lsk_cpu_knn_brute
    for (int64_t qi = b; qi < e; qi++) {
      d.clear();
      for (int64_t i = 0; i < n; i++) {
        const float v = reach_d2(Q[qi], P[i], period);
        if (v < reach_cut(qcut2[qi], pcut2[i], rule)) d.push_back(((uint64_t)lsk::fbits(v) << 32) | (uint32_t)i);
      }
      std::sort(d.begin(), d.end());
      // (offsets come from lsk_cpu_radius_reach_count with the same cutoffs)
      const size_t m = std::min<size_t>(d.size(), (size_t)(offsets[qi + 1] - offsets[qi]));
      for (size_t j = 0; j < m; j++) {
        out_idx[offsets[qi] + (int64_t)j] = (int32_t)(uint32_t)d[j];
        out_d2[offsets[qi] + (int64_t)j] = lsk::bitsf((uint32_t)(d[j] >> 32));
      }
    }
  });
}

// Radius profile: out[q * nb + b] = #{ i : dist2(q, p_i) < cut2s[b] } for the ascending cutoffs
// cut2s[0 .. nb), from one pass over the points per query; period (optional): pdist2 instead.
// A pair goes to shell b0 = #{ b : !(d² < cut2s[b]) } (the cutoffs ascend, so that is the first b
// with d² < cut2s[b]; a NaN d² passes no test and is dropped), and a row is the running sum of
// its shells.
extern "C" void lsk_cpu_radius_profile(const float *pts, int64_t n, const float *qry, int64_t nq,
                                       const float *cut2s, int32_t nb, const float *period, int32_t *out,
                                       int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  if (nb <= 0) return;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t qi = b; qi < e; qi++) {
      int32_t *row = out + qi * nb;
      std::fill(row, row + nb, 0);
      for (int64_t i = 0; i < n; i++) {
        const float v = period ? pdist2(Q[qi], P[i], period) : lsk::dist2(Q[qi], P[i]);
        const float *c = std::partition_point(cut2s, cut2s + nb, [v](float cb) { return !(v < cb); });
        if (c != cut2s + nb) row[c - cut2s]++;
      }
      for (int32_t j = 1; j < nb; j++) row[j] += row[j - 1];
    }
  });
}

// Weighted radius profile: out[q * nb + b] = the sum of w[i] over { i : dist2(q, p_i) < cut2s[b] },
// the walk of lsk_cpu_radius_profile with the point's int64 weight added to its shell in the
// place of 1. Wrapping 64-bit sums: exact whenever the true sums fit (the caller's check).
extern "C" void lsk_cpu_weighted_profile(const float *pts, int64_t n, const float *qry, int64_t nq,
                                         const float *cut2s, int32_t nb, const float *period, const int64_t *w,
                                         int64_t *out, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  if (nb <= 0) return;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<uint64_t> shell((size_t)nb);
    for (int64_t qi = b; qi < e; qi++) {
      std::fill(shell.begin(), shell.end(), (uint64_t)0);
      for (int64_t i = 0; i < n; i++) {
        const float v = period ? pdist2(Q[qi], P[i], period) : lsk::dist2(Q[qi], P[i]);
        const float *c = std::partition_point(cut2s, cut2s + nb, [v](float cb) { return !(v < cb); });
        if (c != cut2s + nb) shell[c - cut2s] += (uint64_t)w[i];
      }
      uint64_t run = 0;
      for (int32_t j = 0; j < nb; j++) {
        run += shell[j];
        out[qi * nb + j] = (int64_t)run;
      }
    }
  });
}

// Anisotropic pair counts along the line-of-sight axis `los` (pair_counts_2d.hip states the
// contract). Per pair the float32 differences q - p (period: their minimum image) give par2 = dl
// * dl of the line-of-sight axis, perp2 = fmaf(db, db, da * da) of the other two in ascending axis
// order, and the canonical d2. mode 0, (rp, pi): the pair's cell is i0 = #{i : !(perp2 < a2[i])},
// j0 = #{j : !(par2 < b2[j])}; mode 1, (s, mu): i0 = #{i : !(d2 < a2[i])}, j0 = #{j : !(par2 <
// b2[j] * d2)} (one float32 product). A pair with i0 == na or j0 == nb is dropped. Every thread
// counts differential cells of its own; out [na, nb] is the 2-D prefix sum of their total.
// w (with wq: optional) null: every pair adds 1; else wq[q] * w[i] (wq null: w[i]), wrapping 64-bit
// sums and products: exact whenever the true sums fit (the caller's check).
// obs (open box: period null, los unused): the line of sight of each pair is the direction from the
// observer obs[0 .. 3) to its midpoint. With l = (q - o) + (p - o) per axis, sl = fmaf(dz, lz,
// fmaf(dy, ly, dx * lx)) and ll = dist2(l): par2 = (sl / ll) * sl, perp2 = d2 - par2 clamped at 0
// from below (a NaN stays a NaN), d2 as before; the cells are the same.
extern "C" void lsk_cpu_pair_sums_2d(const float *pts, int64_t n, const float *qry, int64_t nq, const float *a2,
                                     int32_t na, const float *b2, int32_t nb, int mode, int los, const float *period,
                                     const float *obs, const int64_t *w, const int64_t *wq, int64_t *out,
                                     int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  if (na <= 0 || nb <= 0) return;
  const size_t cells = (size_t)na * (size_t)nb;
  std::vector<uint64_t> total(cells, 0);
  std::mutex mu;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<uint64_t> cell(cells, 0);
    for (int64_t qi = b; qi < e; qi++) {
      const uint64_t fq = wq ? (uint64_t)wq[qi] : 1;
      for (int64_t i = 0; i < n; i++) {
        float d[3] = {Q[qi].x - P[i].x, Q[qi].y - P[i].y, Q[qi].z - P[i].z};
        if (period)
          for (int a = 0; a < 3; a++) d[a] = wrap_diff(d[a], period[a]);
        float par2, va;
        if (obs) {
          const float lx = (Q[qi].x - obs[0]) + (P[i].x - obs[0]), ly = (Q[qi].y - obs[1]) + (P[i].y - obs[1]),
                      lz = (Q[qi].z - obs[2]) + (P[i].z - obs[2]);
          const float sl = fmaf(d[2], lz, fmaf(d[1], ly, d[0] * lx));
          const float ll = lsk::dist2(lx, ly, lz);
          const float d2 = lsk::dist2(d[0], d[1], d[2]);
          par2 = (sl / ll) * sl;
          float perp2 = d2 - par2;
          if (perp2 < 0.f) perp2 = 0.f;
          va = mode == 0 ? perp2 : d2;
        } else {
          const float dl = d[los], da = d[los == 0 ? 1 : 0], db = d[los == 2 ? 1 : 2];
          par2 = dl * dl;
          va = mode == 0 ? fmaf(db, db, da * da) : lsk::dist2(d[0], d[1], d[2]);
        }
        const float *ia = std::partition_point(a2, a2 + na, [va](float c) { return !(va < c); });
        if (ia == a2 + na) continue;
        const float *jb = mode == 0
                              ? std::partition_point(b2, b2 + nb, [par2](float c) { return !(par2 < c); })
                              : std::partition_point(b2, b2 + nb, [par2, va](float c) { return !(par2 < c * va); });
        if (jb == b2 + nb) continue;
        cell[(size_t)(ia - a2) * (size_t)nb + (size_t)(jb - b2)] += w ? fq * (uint64_t)w[i] : 1;
      }
    }
    std::lock_guard<std::mutex> lk(mu);
    for (size_t c = 0; c < cells; c++) total[c] += cell[c];
  });
  for (int32_t i = 0; i < na; i++) {
    uint64_t run = 0;
    for (int32_t j = 0; j < nb; j++) {
      run += total[(size_t)i * nb + j];
      out[(size_t)i * nb + j] = (int64_t)(run + (i ? (uint64_t)out[(size_t)(i - 1) * nb + j] : 0));
    }
  }
}

// lsk_cpu_kth_brute under a period: the k-th smallest pdist2 among those < cut2, else cut2.
extern "C" void lsk_cpu_kth_periodic(const float *pts, int64_t n, const float *qry, int64_t nq, int k, float cut2,
                                     const float *period, float *out_d2, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<float> d;
    d.reserve((size_t)n);
    for (int64_t qi = b; qi < e; qi++) {
      d.clear();
      for (int64_t i = 0; i < n; i++) {
        const float v = pdist2(Q[qi], P[i], period);
        if (v < cut2) d.push_back(v);
      }
      if ((int64_t)d.size() < k) {
        out_d2[qi] = cut2;
      } else {
        std::nth_element(d.begin(), d.begin() + (k - 1), d.end());
        out_d2[qi] = d[(size_t)k - 1];
      }
    }
  });
}

// lsk_cpu_knn_brute under a period, the same selection and tie rule.
extern "C" void lsk_cpu_knn_periodic(const float *pts, int64_t n, const float *qry, int64_t nq, int k, float cut2,
                                     const float *period, int32_t *out_idx, float *out_d2, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    std::vector<uint64_t> d;  // d2 bits << 32 | input row, as lsk_cpu_knn_brute
    d.reserve((size_t)n);
    for (int64_t qi = b; qi < e; qi++) {
      d.clear();
      for (int64_t i = 0; i < n; i++) {
        const float v = pdist2(Q[qi], P[i], period);
        if (v < cut2) d.push_back(((uint64_t)lsk::fbits(v) << 32) | (uint32_t)i);
      }
      const size_t m = std::min<size_t>(d.size(), (size_t)k);
      std::partial_sort(d.begin(), d.begin() + m, d.end());
      for (size_t j = 0; j < (size_t)k; j++) {
        out_idx[qi * k + (int64_t)j] = j < m ? (int32_t)(uint32_t)d[j] : -1;
        out_d2[qi * k + (int64_t)j] = j < m ? lsk::bitsf((uint32_t)(d[j] >> 32)) : cut2;
      }
    }
  });
}

// lsk_cpu_cluster under a period: the same definition with pdist2 for dist2.
extern "C" void lsk_cpu_cluster_periodic(const float *pts, int64_t n, float cut2, int min_pts, const float *period,
                                         int32_t *labels, uint8_t *core, int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  parallel_for(n, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t i = b; i < e; i++) {
      int64_t c = 0;
      for (int64_t j = 0; j < n; j++) c += pdist2(P[i], P[j], period) < cut2;
      core[i] = c >= (int64_t)min_pts;
    }
  });
  std::vector<int32_t> parent((size_t)n);
  for (int64_t i = 0; i < n; i++) parent[(size_t)i] = (int32_t)i;
  auto find = [&](int32_t x) {
    while (parent[(size_t)x] != x) {
      parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
      x = parent[(size_t)x];
    }
    return x;
  };
  for (int64_t i = 0; i < n; i++) {
    if (!core[i]) continue;
    for (int64_t j = i + 1; j < n; j++) {
      if (!core[j] || !(pdist2(P[i], P[j], period) < cut2)) continue;
      const int32_t a = find((int32_t)i), c = find((int32_t)j);
      if (a != c) parent[(size_t)std::max(a, c)] = std::min(a, c);
    }
  }
  for (int64_t i = 0; i < n; i++)
    if (core[i]) labels[i] = find((int32_t)i);
  // (the roots are final: the border points only read them)
  parallel_for(n, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t i = b; i < e; i++) {
      if (core[i]) continue;
      uint64_t best = ~0ull;
      for (int64_t j = 0; j < n; j++) {
        if (!core[j]) continue;
        const float v = pdist2(P[i], P[j], period);
        if (v < cut2) best = std::min(best, ((uint64_t)lsk::fbits(v) << 32) | (uint32_t)j);
      }
      if (best != ~0ull)
        labels[i] = labels[(size_t)(uint32_t)best];
      else
        labels[i] = min_pts == 1 ? (int32_t)i : -1;
    }
  });
}

extern "C" void lsk_cpu_count_below(const float *pts, int64_t n, const float *qry,
                                    const float *thr, int nq, unsigned long long *counts,
                                    int nthreads) {
  const vec3f *P = (const vec3f *)pts;
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t j = b; j < e; j++) {
      unsigned long long lt = 0, le = 0;
      for (int64_t i = 0; i < n; i++) {
        const float v = lsk::dist2(Q[j], P[i]);
        lt += v < thr[2 * j];
        le += v < thr[2 * j + 1];
      }
      counts[2 * j] += lt;
      counts[2 * j + 1] += le;
    }
  });
}

extern "C" void lsk_cpu_kth_kdtree(const float *pts, int64_t n, const float *qry, int64_t nq,
                                   int k, float cut2, float *out_d2, int nthreads) {
  KdTree t;
  t.pts.assign((const vec3f *)pts, (const vec3f *)pts + n);
  if (n > 0) t.nodes.reserve((size_t)(2 * n / KdTree::kLeaf + 16)), t.build(0, n);
  const vec3f *Q = (const vec3f *)qry;
  parallel_for(nq, nthreads, [&](int64_t b, int64_t e) {
    KHeap heap;
    std::vector<std::pair<int64_t, float>> stack;
    for (int64_t qi = b; qi < e; qi++) out_d2[qi] = t.query(Q[qi], k, cut2, heap, stack);
  });
}

extern "C" void lsk_cpu_bounds(const float *pts, int64_t n, float *box, int nthreads) {
  const float inf = std::numeric_limits<float>::infinity();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  std::vector<std::array<float, 6>> part;
  std::mutex mu;
  parallel_for(n, nthreads, [&](int64_t b, int64_t e) {
    float l[3] = {inf, inf, inf}, h[3] = {-inf, -inf, -inf};
    for (int64_t i = b; i < e; i++)
      for (int a = 0; a < 3; a++) {
        l[a] = std::min(l[a], pts[3 * i + a]);
        h[a] = std::max(h[a], pts[3 * i + a]);
      }
    std::lock_guard<std::mutex> g(mu);
    for (int a = 0; a < 3; a++) {
      lo[a] = std::min(lo[a], l[a]);
      hi[a] = std::max(hi[a], h[a]);
    }
  });
  for (int a = 0; a < 3; a++) {
    box[a] = lo[a];
    box[3 + a] = hi[a];
  }
}

extern "C" void lsk_cpu_morton(const float *pts, int64_t n, const float *origin, float scale,
                               uint32_t *keys, int curve, int nthreads) {
  parallel_for(n, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t i = b; i < e; i++) {
      uint32_t ix = lsk::morton_quant(pts[3 * i + 0], origin[0], scale);
      uint32_t iy = lsk::morton_quant(pts[3 * i + 1], origin[1], scale);
      uint32_t iz = lsk::morton_quant(pts[3 * i + 2], origin[2], scale);
      keys[i] = lsk::curve3(curve, ix, iy, iz);
    }
  });
}

extern "C" void lsk_cpu_halo_mask(const float *pts, int64_t n, const float *boxes,
                                  const int64_t *box_offsets, int nsets, int skip_set,
                                  uint64_t *mask, int nthreads) {
  parallel_for(n, nthreads, [&](int64_t b, int64_t e) {
    for (int64_t i = b; i < e; i++) {
      vec3f p{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
      uint64_t m = 0;
      for (int s = 0; s < nsets && s < 64; s++) {
        if (s == skip_set) continue;
        for (int64_t j = box_offsets[s]; j < box_offsets[s + 1]; j++) {
          const float *bx = boxes + 8 * j;
          float d2 = lsk::box_dist2(p, vec3f{bx[0], bx[1], bx[2]}, vec3f{bx[4], bx[5], bx[6]});
          if (d2 < bx[3]) {
            m |= (1ull << s);
            break;
          }
        }
      }
      mask[i] = m;
    }
  });
}
