"""Tensor-level wrappers around the gfx950 kernels (and their CPU counterparts).

Every function takes/returns torch tensors. CUDA (ROCm) tensors run the hand-written
HIP kernels of ``csrc/hip`` on torch's current stream; CPU tensors run the C++ host
runtime (``csrc/host``) or plain torch — that path exists for the CPU oracle, the
``--device cpu`` mode and multi-process ``gloo`` tests. A CUDA tensor never falls back
to the CPU path: if the kernel library is missing the call raises.

uint32 data (Morton keys, indices) is stored in ``torch.int32`` tensors (same bits).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from .. import _native
from .._native import GridView, KnnArgs, TreeView, check

BUCKET = 64
PAD_POINTS = 64  # readable padding required after point arrays read by the knn kernel


def _nthreads() -> int:
    return max(1, min(16, os.cpu_count() or 1))


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def is_gpu(t: torch.Tensor) -> bool:
    return t.device.type == "cuda"


# --------------------------------------------------------------------------- bounds
def bounds(pts: torch.Tensor) -> torch.Tensor:
    """AABB + Morton cube of an [n,3] float32 tensor -> [8] (lo.xyz, hi.xyz, scale, extent)."""
    n = pts.shape[0]
    if is_gpu(pts):
        lib = _native.hip()
        box = torch.empty(8, dtype=torch.float32, device=pts.device)
        ws = torch.empty(lib.lsk_hip_bounds_ws_bytes(n) // 4 + 1, dtype=torch.float32, device=pts.device)
        check(lib.lsk_hip_bounds(_ptr(pts), n, _ptr(box), _ptr(ws), _stream(pts)), "bounds")
        return box
    box = torch.empty(8, dtype=torch.float32)
    _native.host().lsk_cpu_bounds(_ptr(pts.contiguous()), n, _ptr(box), _nthreads())
    return box_finalize(box)


def box_finalize(box: torch.Tensor) -> torch.Tensor:
    """Recompute the Morton cube (box[6:8]) from box[0:6]."""
    if is_gpu(box):
        check(_native.hip().lsk_hip_box_finalize(_ptr(box), _stream(box)), "box_finalize")
        return box
    lo, hi = box[0:3], box[3:6]
    ex = float(torch.max(hi - lo)) if bool(torch.all(torch.isfinite(box[0:6]))) else 0.0
    ok = ex > 0 and math.isfinite(ex)
    box[6] = 1024.0 / ex if ok else 0.0
    box[7] = ex if ok else 0.0
    return box


# --------------------------------------------------------------------------- curve keys + sort
CURVES = {"morton": 0, "hilbert": 1}
# Space-filling curve of the sort keys: Hilbert runs are spatially much tighter than
# Z-order runs (fewer tree nodes and quarters per query, smaller halos); Morton kept
# for A/B measurements (LSKNN_CURVE=morton).
CURVE = os.environ.get("LSKNN_CURVE", "hilbert")


def morton(pts: torch.Tensor, box: torch.Tensor, with_iota: bool = True, curve: str | None = None):
    """30-bit space-filling-curve keys (Hilbert by default, `CURVE`) of pts in the cube
    of `box`; returns (keys, iota)."""
    cid = CURVES[curve or CURVE]
    n = pts.shape[0]
    keys = torch.empty(n, dtype=torch.int32, device=pts.device)
    vals = torch.empty(n, dtype=torch.int32, device=pts.device) if with_iota else None
    if is_gpu(pts):
        check(_native.hip().lsk_hip_morton(_ptr(pts), n, _ptr(box), _ptr(keys), _ptr(vals), cid,
                                           _stream(pts)), "morton")
        return keys, vals
    b = box.detach().cpu()
    origin = b[0:3].contiguous()
    _native.host().lsk_cpu_morton(_ptr(pts.contiguous()), n, _ptr(origin), C.c_float(float(b[6])),
                                  _ptr(keys), cid, _nthreads())
    if vals is not None:
        vals.copy_(torch.arange(n, dtype=torch.int32))
    return keys, vals


def morton_into(pts: torch.Tensor, box: torch.Tensor, keys: torch.Tensor, vals: torch.Tensor | None,
                base: int, flag: torch.Tensor | None = None, curve: str | None = None) -> None:
    """GPU: keys of pts (and vals = base + i) written into the given (slice) tensors; with
    a device int32 `flag` nothing is written unless flag != 0 (decided on the device)."""
    check(_native.hip().lsk_hip_morton_ex(_ptr(pts), pts.shape[0], _ptr(box), _ptr(keys),
                                          _ptr(vals) if vals is not None else None, CURVES[curve or CURVE],
                                          int(base), _ptr(flag) if flag is not None else None,
                                          _stream(pts)), "morton_ex")


def sort_pairs(keys: torch.Tensor, vals: torch.Tensor, key_bits: int = 30):
    """Stable sort of (key, value) int32 pairs by the low `key_bits` bits of key (unsigned)."""
    n = keys.shape[0]
    if not is_gpu(keys):
        k64 = keys.to(torch.int64) & ((1 << 32) - 1)
        if key_bits < 32:
            k64 = k64 & ((1 << key_bits) - 1)
        order = torch.sort(k64, stable=True).indices
        return keys[order], vals[order]
    lib = _native.hip()
    ka = torch.empty_like(keys)
    va = torch.empty_like(vals)
    ws = torch.empty(lib.lsk_hip_sort_ws_bytes(n), dtype=torch.uint8, device=keys.device)
    alt = C.c_int(0)
    check(lib.lsk_hip_sort_pairs(_ptr(keys), _ptr(vals), _ptr(ka), _ptr(va), n, key_bits, _ptr(ws),
                                 C.byref(alt), _stream(keys)), "sort_pairs")
    return (ka, va) if alt.value else (keys, vals)


def sort_keys_iota(keys: torch.Tensor, key_bits: int = 30):
    """sort_pairs(keys, arange(n)) without the arange: the GPU sort's first pass generates
    the values (no 4-byte-per-point array written and read back)."""
    n = keys.shape[0]
    if not is_gpu(keys):
        return sort_pairs(keys, torch.arange(n, dtype=torch.int32), key_bits)
    lib = _native.hip()
    vals = torch.empty_like(keys)
    ka = torch.empty_like(keys)
    va = torch.empty_like(keys)
    ws = torch.empty(lib.lsk_hip_sort_ws_bytes(n), dtype=torch.uint8, device=keys.device)
    alt = C.c_int(0)
    check(lib.lsk_hip_sort_keys_iota(_ptr(keys), _ptr(vals), _ptr(ka), _ptr(va), n, key_bits, _ptr(ws),
                                     C.byref(alt), _stream(keys)), "sort_keys_iota")
    return (ka, va) if alt.value else (keys, vals)


def sort_keys_iota_gather(keys: torch.Tensor, points: torch.Tensor, key_bits: int = 30, pad: int = 0):
    """sort_keys_iota + the points in sorted order (`pad` extra zero rows), gathered by the
    sort's last pass instead of a separate gather3 over the permutation. Returns (sorted
    keys, permutation, sorted points)."""
    n = keys.shape[0]
    if not is_gpu(keys) or n < 2:
        sk, perm = sort_keys_iota(keys, key_bits)
        return sk, perm, gather3(points, perm, pad=pad)
    lib = _native.hip()
    vals = torch.empty_like(keys)
    ka = torch.empty_like(keys)
    va = torch.empty_like(keys)
    ws = torch.empty(lib.lsk_hip_sort_ws_bytes(n), dtype=torch.uint8, device=keys.device)
    pts = torch.empty((n + pad, 3), dtype=torch.float32, device=keys.device)
    if pad:
        pts[n:].zero_()
    points = points.contiguous()
    alt = C.c_int(0)
    check(lib.lsk_hip_sort_keys_iota_gather(_ptr(keys), _ptr(vals), _ptr(ka), _ptr(va), n, key_bits, _ptr(ws),
                                            C.byref(alt), _ptr(points), _ptr(pts), _stream(keys)),
          "sort_keys_iota_gather")
    return ((ka, va) if alt.value else (keys, vals)) + (pts,)


def key_census(skeys: torch.Tensor, run: int) -> tuple[torch.Tensor, torch.Tensor]:
    """One device pass over sorted keys: (int64 [11] level counts as key_levels_dev, int32
    [1] heavy flag: some key equals the one `run` positions earlier). No host read."""
    cnt = torch.zeros(11, dtype=torch.int64, device=skeys.device)
    heavy = torch.zeros(1, dtype=torch.int32, device=skeys.device)
    check(_native.hip().lsk_hip_key_census(_ptr(skeys), skeys.shape[0], _ptr(cnt), int(run), _ptr(heavy),
                                           _stream(skeys)), "key_census")
    return cnt, heavy


def segment_bounds(p: torch.Tensor, seg: torch.Tensor, nseg: int):
    """Per-segment AABB of GPU points p [m,3] with contiguous segment ids seg (int32,
    non-decreasing runs) -> (lo, hi) [nseg, 3]."""
    lo = torch.empty((nseg, 3), dtype=torch.float32, device=p.device)
    hi = torch.empty((nseg, 3), dtype=torch.float32, device=p.device)
    check(_native.hip().lsk_hip_segment_bounds(_ptr(p.contiguous()), _ptr(seg.contiguous()), p.shape[0], nseg,
                                               _ptr(lo), _ptr(hi), _stream(p)), "segment_bounds")
    return lo, hi


def gather3(src: torch.Tensor, idx: torch.Tensor, pad: int = 0) -> torch.Tensor:
    """dst[i] = src[idx[i]] for float3 rows; dst gets `pad` extra zero rows."""
    n = idx.shape[0]
    dst = torch.empty((n + pad, 3), dtype=torch.float32, device=src.device)
    if pad:
        dst[n:].zero_()
    if is_gpu(src):
        check(_native.hip().lsk_hip_gather3(_ptr(src), _ptr(idx), n, _ptr(dst), _stream(src)), "gather3")
    else:
        dst[:n] = src[idx.to(torch.int64)]
    return dst


def scatter1(src: torch.Tensor, idx: torch.Tensor, out: torch.Tensor, finalize: bool) -> torch.Tensor:
    """out[idx[i]] = f(src[i]) with f = sqrt-unless-inf when finalize."""
    n = src.shape[0]
    if is_gpu(src):
        check(_native.hip().lsk_hip_scatter1(_ptr(src), _ptr(idx), n, _ptr(out), int(finalize), _stream(src)),
              "scatter1")
    else:
        v = finalize_distances(src) if finalize else src
        out[idx.to(torch.int64)] = v
    return out


def finalize_distances(d2: torch.Tensor) -> torch.Tensor:
    """sqrt of the k-th squared distance unless it is +inf (reference extractFinalResult)."""
    if is_gpu(d2):
        out = torch.empty_like(d2)
        check(_native.hip().lsk_hip_finalize(_ptr(d2), d2.shape[0], _ptr(out), _stream(d2)), "finalize")
        return out
    # torch's float32 CPU sqrt is not correctly rounded (vectorised approximation);
    # sqrt in float64 then one rounding to float32 is (IEEE sqrtf, as on the GPU).
    return torch.where(torch.isinf(d2), d2, torch.sqrt(d2.double()).float())


# --------------------------------------------------------------------------- tree
def tree_depth(n: int) -> int:
    nb = (n + BUCKET - 1) // BUCKET
    d = 0
    while (1 << d) < nb:
        d += 1
    return d


def build_tree(sorted_pts: torch.Tensor, n: int) -> tuple[torch.Tensor, torch.Tensor, int]:
    """Bucket tree over the first n rows of sorted_pts -> (nodes [2^(D+1), 8],
    quarter boxes [2^D * 4, 8], depth)."""
    depth = tree_depth(n)
    slots = 1 << depth
    if is_gpu(sorted_pts):
        nodes = torch.empty((2 * slots, 8), dtype=torch.float32, device=sorted_pts.device)
        qnodes = torch.empty((4 * slots, 8), dtype=torch.float32, device=sorted_pts.device)
        check(_native.hip().lsk_hip_build_tree(_ptr(sorted_pts), n, _ptr(nodes), _ptr(qnodes),
                                               _stream(sorted_pts)), "build_tree")
        return nodes, qnodes, depth
    inf = float("inf")
    lo = torch.full((slots * BUCKET, 3), inf)
    hi = torch.full((slots * BUCKET, 3), -inf)
    lo[:n] = sorted_pts[:n]
    hi[:n] = sorted_pts[:n]
    qnodes = torch.zeros((4 * slots, 8), dtype=torch.float32)
    qnodes[:, 0:3] = lo.view(4 * slots, 16, 3).amin(dim=1)
    qnodes[:, 4:7] = hi.view(4 * slots, 16, 3).amax(dim=1)
    nodes = torch.zeros((2 * slots, 8), dtype=torch.float32)
    nodes[slots:, 0:3] = lo.view(slots, BUCKET, 3).amin(dim=1)
    nodes[slots:, 4:7] = hi.view(slots, BUCKET, 3).amax(dim=1)
    for level in range(depth - 1, -1, -1):
        a = 1 << level
        ch = nodes[2 * a: 4 * a].view(a, 2, 8)
        nodes[a:2 * a, 0:3] = torch.minimum(ch[:, 0, 0:3], ch[:, 1, 0:3])
        nodes[a:2 * a, 4:7] = torch.maximum(ch[:, 0, 4:7], ch[:, 1, 4:7])
        nodes[a:2 * a, 3] = torch.fmax(ch[:, 0, 3], ch[:, 1, 3])
    return nodes, qnodes, depth


def tree_set_radii(nodes: torch.Tensor, n: int, d2_sorted: torch.Tensor) -> torch.Tensor:
    """Store per-node max k-th squared radius (lo.w) of the queries below each node."""
    if is_gpu(nodes):
        check(_native.hip().lsk_hip_tree_set_radii(_ptr(nodes), n, _ptr(d2_sorted), _stream(nodes)),
              "tree_set_radii")
        return nodes
    depth = tree_depth(n)
    slots = 1 << depth
    r = torch.zeros(slots * BUCKET, dtype=torch.float32)
    d2 = d2_sorted[:n]
    # an unresolved (NaN) radius widens the bound to +inf, as leaf_radius_kernel does: amax
    # would keep the NaN, and box_dist2 < NaN then drops every candidate of the subtree
    r[:n] = torch.where(d2 != d2, torch.full_like(d2, math.inf), d2)
    nodes[slots:, 3] = r.view(slots, BUCKET).amax(dim=1)
    return _levelup_radii(nodes, depth)


def _levelup_radii(nodes: torch.Tensor, depth: int) -> torch.Tensor:
    """CPU: inner-node radii (lo.w) = max of the children's, up to node 1 (fmaxf as
    levelup_kernel: a NaN never replaces a number)."""
    for level in range(depth - 1, -1, -1):
        a = 1 << level
        ch = nodes[2 * a: 4 * a].view(a, 2, 8)
        nodes[a:2 * a, 3] = torch.fmax(ch[:, 0, 3], ch[:, 1, 3])
    return nodes


# --------------------------------------------------------------------------- kNN
def radius_hint(box: torch.Tensor, n_total: int, k: int) -> torch.Tensor:
    """Device [1] float32: uniform-density k-th squared distance estimate of a GPU box."""
    out = torch.empty(1, dtype=torch.float32, device=box.device)
    check(_native.hip().lsk_hip_radius_hint(_ptr(box), int(n_total), int(k), _ptr(out), _stream(box)),
          "radius_hint")
    return out


ROWS_MAX_K = 65535  # 16-bit histogram bins of knn_rows; larger k go to the exact kernel
FAIL_CAP_OVERRIDE: int | None = None  # tests: force failure-list overflows (whole reruns)


def fail_capacity(work: int) -> int:
    """Capacity of the failure list of one knn_rows launch over `work` queries: all of
    them up to 64M, then 1/16 of them (a failure count above it makes the host rerun the
    whole query on the exact kernel, see knn_engine.query)."""
    if FAIL_CAP_OVERRIDE is not None:
        return max(1, min(work, FAIL_CAP_OVERRIDE))
    return max(1, min(work, max(1 << 26, work >> 4)))


# Foreign queries (knn_gpu qbucket): the rows kernel places its first range from the located
# bucket's points (True) or from the density hint alone (False: the A/B of that estimate).
FOREIGN_ESTIMATE = True


def locate_groups(sorted_qkeys: torch.Tensor, nq: int, bucket_keys: torch.Tensor) -> torch.Tensor:
    """int32 [ceil(nq / 64)]: for every group of 64 curve-sorted queries, the last bucket of
    an index whose first key (bucket_keys, non-decreasing) is <= the group's median key."""
    ng = (nq + BUCKET - 1) // BUCKET
    nb = bucket_keys.shape[0]
    if not is_gpu(sorted_qkeys):
        out = torch.zeros(ng, dtype=torch.int32)
        if ng and nb:
            mask = (1 << 32) - 1
            q0 = torch.arange(ng, dtype=torch.int64) * BUCKET
            med = sorted_qkeys.to(torch.int64)[q0 + torch.clamp(nq - q0, max=BUCKET) // 2] & mask
            pos = torch.searchsorted(bucket_keys.to(torch.int64) & mask, med, right=True) - 1
            out.copy_(pos.clamp_(min=0))
        return out
    out = torch.empty(ng, dtype=torch.int32, device=sorted_qkeys.device)
    check(_native.hip().lsk_hip_locate_groups(_ptr(sorted_qkeys), int(nq), _ptr(bucket_keys), int(nb), _ptr(out),
                                              _stream(sorted_qkeys)), "locate_groups")
    return out


class FailWord:
    """Always-on failure word of one k-NN launch: count (device int32) of the queries the
    16-bit kernel handed to the exact backstop, and the list capacity. Reading it syncs."""

    def __init__(self, count: torch.Tensor | None, cap: int):
        self.count = count
        self.cap = cap
        self._host = None
        self._ev = None
        self._gate = None
        self.flist = None

    def stage(self, gate: torch.Tensor | None = None) -> None:
        """Queue the word's copy to pinned host memory on the current stream (right behind
        the launch): a later value() waits for this launch only, not for work queued on
        the stream after it. `gate` (the device grid decision, int32 [1]) is staged with it
        (gate_value()): a .item() would wait for everything queued on the stream since."""
        if self.count is None or self.count.device.type != "cuda":
            return
        self._host = torch.empty(2, dtype=torch.int32, pin_memory=True)
        self._host[0:1].copy_(self.count.view(torch.int32), non_blocking=True)
        if gate is not None:
            self._host[1:2].copy_(gate.view(-1)[:1].to(torch.int32), non_blocking=True)
            self._gate = gate
        self._ev = torch.cuda.Event()
        self._ev.record()

    def gate_value(self, gate: torch.Tensor) -> int:
        """The staged grid decision (stage(gate)), else a direct read."""
        if self._gate is gate and self._ev is not None:
            self._ev.synchronize()
            return int(self._host[1])
        return int(gate.item())

    def value(self) -> int:
        # the kernels count in uint32 (a count >= 2^31 must not read as negative)
        if self.count is None:
            return 0
        if self._ev is not None:
            self._ev.synchronize()
            return int(self._host[0]) & 0xFFFFFFFF
        return int(self.count.item()) & 0xFFFFFFFF

    def overflowed(self) -> bool:
        return self.value() > self.cap


def knn_gpu(qpts: torch.Tensor, nq: int, trees: list, k: int, cut2: float,
            r_hint2: float | torch.Tensor,
            out_d2: torch.Tensor, groups: torch.Tensor | None = None, ngroups: int = 0,
            stats: torch.Tensor | None = None, qstatus: torch.Tensor | None = None,
            seed: int = 0, impl: str = "rows", init_d2: torch.Tensor | None = None,
            out_perm: torch.Tensor | None = None, out_final: torch.Tensor | None = None,
            debug_fail_mod: int = 0, grid=None, ngroups_dev: torch.Tensor | None = None,
            expect_grid: bool = True, short_list: bool = False, chunks: int = 1, grid2=None,
            qrot: torch.Tensor | None = None, qbucket: torch.Tensor | None = None) -> FailWord:
    """k-th squared distance for sorted queries against up to two bucket trees.

    trees: list of (sorted_pts_padded, nodes, qnodes, n, depth). impl: "rows" (the
    production kernel: 4 x 16-query rows, 16-bit LDS histograms; every query it cannot
    resolve exactly goes to the failure list and is recomputed by the exact kernel in the
    same stream, no host round trip) or "exact" (the wave-per-query 32-bit backstop for
    every query; also used for k > 65535). seed > 0 declares that the queries are
    trees[0]'s points in tree order (pass 1 starts from neighbour buckets).
    init_d2 (optional, [nq]): a known upper bound of every query's k-th squared distance
    (e.g. the local result before a halo re-query) that places the first range.
    out_perm / out_final (optional, fused scatter): the kernels also write
    out_final[out_perm[q]] = final distance; out_d2 may then be None.
    debug_fail_mod (tests): the rows kernel also fails every query q with q % mod == 0.
    ngroups_dev (optional, with groups): int32 [1] on the device, the list's length
    (ngroups is then only the launch's upper bound).
    expect_grid (with a gate): which kernel the gate is expected to pick — that one gets the
    full launch, the other its persistent strided form (a small grid whose waves return at
    once when the gate rejects it; a misprediction costs speed, never exactness).
    short_list (with ngroups_dev): the device-side list is expected far shorter than
    ngroups (a rank's boundary groups): the kernel that runs takes its persistent strided
    form at full occupancy instead of one wave per possible group (most would be
    dispatched only to return: ~16 ms per 1M-block launch).
    chunks > 1: the pass goes out as that many launches over consecutive wave ranges —
    kernel boundaries at which the high-priority streams' kernels (the next set's
    redistribution, the halo exchange) get CU slots: a running k-NN grid keeps every slot
    until its last workgroup is dispatched.
    grid (impl "grid"): (slots, level, box, inf4[, gate]) of knn_engine.GridIndex — the
    cell-grid candidate source of knn_grid.hip for one tree whose points are the queries
    (or, with qbucket, any queries: the walk starts from the wave's box by arithmetic;
    same failure list and backstop as "rows"); with a device gate (int32 [1]) the grid
    kernel runs iff gate == 1 and knn_rows iff gate == 0.
    grid2 (impl "grid", two trees: the halo re-query): the second tree's grid (slots, level,
    box, inf4) — knn_grid2 walks both grids; init_d2 is allowed then.
    qrot (one tree, rows / exact): the queries in the rotated frame trees[0]'s boxes were
    built in (knn_engine.flat_frame); box tests use it, distances qpts.
    qbucket (int32 [ceil(nq / 64)], locate_groups): the queries are NOT trees[0]'s points
    (foreign queries, knn_engine.query_points) — one unrotated tree, no group list; the rows
    / grid kernels run their foreign forms: the walk's own bucket and the first range come
    from the located bucket (FOREIGN_ESTIMATE), nothing from neighbouring queries. None:
    the queries are the tree's points, as ever.
    Returns the launch's FailWord.
    """
    if (out_perm is None) != (out_final is None):
        raise ValueError("knn_gpu: out_perm and out_final go together")
    if out_perm is not None and (out_perm.shape[0] < nq or out_perm.dtype != torch.int32
                                 or not out_perm.is_contiguous() or out_final.dtype != torch.float32):
        raise ValueError("knn_gpu: out_perm must be int32 [>= nq], out_final float32")
    if impl not in ("rows", "exact", "grid"):
        raise ValueError(f"knn_gpu: impl must be rows, exact or grid, not {impl!r}")
    if impl == "grid" and (grid is None or len(trees) != (2 if grid2 is not None else 1)
                           or (grid2 is None and init_d2 is not None)):
        raise ValueError("knn_gpu: impl grid needs a grid and one tree (no init_d2), or two trees and grid2")
    a = KnnArgs()
    a.qpts = _ptr(qpts)
    a.nq = nq
    a.groups = _ptr(groups)
    a.ngroups = ngroups
    a.ngroups_dev = _ptr(ngroups_dev) if groups is not None else None
    for i, (pts, nodes, qnodes, n, depth) in enumerate(trees):
        a.tree[i] = TreeView(_ptr(pts), _ptr(nodes), _ptr(qnodes), n, depth, 0)
    a.ntrees = len(trees)
    a.k = k
    a.cut2 = cut2
    if isinstance(r_hint2, torch.Tensor):
        # device value (K.radius_hint): parked in the unused node 0 of tree 0, which the
        # kernel reads when r_hint2 < 0 — no host round trip, no extra kernel argument
        trees[0][1].view(-1)[3:4].copy_(r_hint2.view(-1)[:1])
        a.r_hint2 = -1.0
    else:
        a.r_hint2 = max(float(r_hint2), 0.0)
    a.out_d2 = _ptr(out_d2)
    a.stats = _ptr(stats)
    a.qstatus = _ptr(qstatus)
    a.seed = seed
    a.init_d2 = _ptr(init_d2)
    if qrot is not None and (impl == "grid" or len(trees) != 1):
        raise ValueError("knn_gpu: qrot needs one tree and the rows / exact kernel")
    a.qrot = _ptr(qrot)
    a.out_perm = _ptr(out_perm)
    a.out_final = _ptr(out_final)
    a.debug_fail_mod = int(debug_fail_mod)
    if qbucket is not None:
        if len(trees) != 1 or qrot is not None or groups is not None or grid2 is not None:
            raise ValueError("knn_gpu: foreign queries (qbucket) take one unrotated tree and no group list")
        if qbucket.dtype != torch.int32 or not qbucket.is_contiguous() or qbucket.shape[0] < (nq + BUCKET - 1) // BUCKET:
            raise ValueError("knn_gpu: qbucket must be int32 [>= ceil(nq / 64)]")
        a.qbucket = _ptr(qbucket)
        a.foreign = 1 if FOREIGN_ESTIMATE else 2
    lib = _native.hip()
    st = _stream(qpts)
    if impl == "exact" or k > ROWS_MAX_K:
        check(lib.lsk_hip_knn_exact(C.byref(a), None, None, 0, st), "knn_exact")
        return FailWord(None, 0)
    work = ngroups * BUCKET if groups is not None else nq
    cap = fail_capacity(work)
    count = torch.zeros(1, dtype=torch.int32, device=qpts.device)
    flist = torch.empty(cap, dtype=torch.int32, device=qpts.device)
    a.fail_list = _ptr(flist)
    a.fail_count = _ptr(count)
    a.fail_cap = cap
    full = 2 if short_list and groups is not None and ngroups_dev is not None else 0
    # a short device-counted list runs persistent waves that take their groups from a work
    # queue (one zeroed counter per launch): re-query groups differ widely in cost, and a
    # static stride left the halo re-query at 9.1 vs 6.9 ms with the exact-size launch
    # (1B / 8 ranks, scripts/rank_replay.py)
    wqs = torch.zeros(2 * max(1, int(chunks)), dtype=torch.int32, device=qpts.device) if full else None
    nw = ngroups if groups is not None else (nq + BUCKET - 1) // BUCKET
    chunks = max(1, min(int(chunks), nw))
    # the pass as `chunks` consecutive launches over wave ranges (0 = to the end)
    spans = [(0, 0)] if chunks == 1 else [(nw * c // chunks, nw * (c + 1) // chunks) for c in range(chunks)]
    def _wq(i: int, on: bool):
        a.wq = _ptr(wqs[i:i + 1]) if on and wqs is not None else None

    if impl == "grid":
        slots, level, gbox, inf4 = grid[:4]
        gate = grid[4] if len(grid) > 4 else None
        gv = GridView(_ptr(slots), None, _ptr(gbox), _ptr(inf4), int(level), 0)
        gv2 = GridView(_ptr(grid2[0]), None, _ptr(grid2[2]), _ptr(grid2[3]), int(grid2[1]), 0) if grid2 is not None else None
        for ci, (a.wave_base, a.wave_end) in enumerate(spans):
            if gate is not None:
                # the device decides (lsk_hip_grid_decide): both kernels are queued, the one
                # not chosen returns at its first instruction (no host read, graph-capturable)
                a.gate = _ptr(gate)
                a.gate_on = 1
                a.pad2 = full if expect_grid else 1
            else:
                a.pad2 = full
            _wq(2 * ci, a.pad2 == 2)
            if gv2 is not None:
                check(lib.lsk_hip_knn_grid2(C.byref(a), C.byref(gv), C.byref(gv2), st), "knn_grid2")
            else:
                check(lib.lsk_hip_knn_grid(C.byref(a), C.byref(gv), st), "knn_grid")
            if gate is not None:
                a.gate_on = 0
                a.pad2 = 1 if expect_grid else full
                _wq(2 * ci + 1, a.pad2 == 2)
                check(lib.lsk_hip_knn_rows(C.byref(a), st), "knn_rows")
            a.gate = None
            a.pad2 = 0
    else:
        for ci, (a.wave_base, a.wave_end) in enumerate(spans):
            a.pad2 = full
            _wq(ci, a.pad2 == 2)
            check(lib.lsk_hip_knn_rows(C.byref(a), st), "knn_rows")
            a.pad2 = 0
    a.wave_base = a.wave_end = 0
    a.wq = None
    # exact backstop over the failure list (device-side count: empty list = short no-op)
    check(lib.lsk_hip_knn_exact(C.byref(a), _ptr(flist), _ptr(count), cap, st), "knn_exact")
    fw = FailWord(count, cap)
    fw.flist = flist  # (debugging: the failed queries' positions, flist[:count])
    return fw


# --------------------------------------------------------------------------- cell grid
def key_levels(skeys: torch.Tensor) -> list[int]:
    """Distinct cells of each octree level 0..10 among sorted 30-bit curve keys (one
    device pass + one 88-byte read): [1, d1, ..., d10]."""
    n = skeys.shape[0]
    if n == 0:
        return [0] * 11
    cnt = torch.empty(11, dtype=torch.int64, device=skeys.device)
    check(_native.hip().lsk_hip_key_levels(_ptr(skeys), n, _ptr(cnt), _stream(skeys)), "key_levels")
    c = cnt.cpu().tolist()
    return [1] + [int(c[l]) + 1 for l in range(1, 11)]


def grid_build(sorted_pts: torch.Tensor, sorted_keys: torch.Tensor, n: int, box: torch.Tensor, level: int):
    """Grandchild runs of the octree grid over the curve-sorted points (knn_grid.hip): every
    level-`level` cell has 64 slots (its level+2 grandchildren in curve order), each
    (start, end, packed coords, 0) -> int32 [8^level * 64, 4]."""
    dev = sorted_pts.device
    slots = torch.empty((64 << (3 * level), 4), dtype=torch.int32, device=dev)
    check(_native.hip().lsk_hip_grid_build(_ptr(sorted_pts), _ptr(sorted_keys), n, _ptr(box), level, _ptr(slots),
                                           _stream(sorted_pts)), "grid_build")
    return slots


def key_levels_dev(skeys: torch.Tensor) -> torch.Tensor:
    """key_levels without the host read: int64 [11] on the device, counts[l] = distinct
    level-l cells - 1 (the raw lsk_hip_key_levels output)."""
    cnt = torch.zeros(11, dtype=torch.int64, device=skeys.device)
    if skeys.shape[0] > 0:
        check(_native.hip().lsk_hip_key_levels(_ptr(skeys), skeys.shape[0], _ptr(cnt), _stream(skeys)),
              "key_levels")
    return cnt


def grid_sq_dev(slots: torch.Tensor) -> torch.Tensor:
    """grid_sq without the host read: int64 [1] on the device."""
    out = torch.zeros(1, dtype=torch.int64, device=slots.device)
    check(_native.hip().lsk_hip_grid_sq(_ptr(slots), slots.shape[0], _ptr(out), _stream(slots)), "grid_sq")
    return out


def grid_decide(counts: torch.Tensor, sq: torch.Tensor, n: int, g: int, crowd: float, check_uniform: bool):
    """Device flag int32 [1]: 1 iff the grid applies (lsk_hip_grid_decide), no host read."""
    gate = torch.empty(1, dtype=torch.int32, device=counts.device)
    check(_native.hip().lsk_hip_grid_decide(_ptr(counts), _ptr(sq), n, g, C.c_float(crowd), int(check_uniform),
                                            _ptr(gate), _stream(counts)), "grid_decide")
    return gate


def grid_sq(slots: torch.Tensor) -> int:
    """Sum over grid slots of population^2 (host read)."""
    out = torch.zeros(1, dtype=torch.int64, device=slots.device)
    check(_native.hip().lsk_hip_grid_sq(_ptr(slots), slots.shape[0], _ptr(out), _stream(slots)), "grid_sq")
    return int(out.item())


def kth_cpu(points: torch.Tensor, queries: torch.Tensor, k: int, cut2: float, method: str = "kdtree") -> torch.Tensor:
    """CPU oracle: k-th squared distance of each query among points (self counted if present)."""
    pts = points.contiguous().float()
    q = queries.contiguous().float()
    out = torch.empty(q.shape[0], dtype=torch.float32)
    f = _native.host().lsk_cpu_kth_kdtree if method == "kdtree" else _native.host().lsk_cpu_kth_brute
    f(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], int(k), C.c_float(cut2), _ptr(out), _nthreads())
    return out


def knn_cpu(points: torch.Tensor, queries: torch.Tensor, k: int, cut2: float) -> tuple[torch.Tensor, torch.Tensor]:
    """CPU oracle of the neighbour lists (brute force): (idx int32 [nq, k], d2 float32 [nq, k]),
    per query the first k of {(dist2, row) : dist2 < cut2} in ascending (dist2, row) order;
    unfilled slots hold -1 / cut2. d2[:, k - 1] equals kth_cpu."""
    if k < 1:
        raise ValueError("knn_cpu: k must be at least 1")
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    idx = torch.empty((q.shape[0], k), dtype=torch.int32)
    d2 = torch.empty((q.shape[0], k), dtype=torch.float32)
    _native.host().lsk_cpu_knn_brute(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], int(k), C.c_float(cut2),
                                     _ptr(idx), _ptr(d2), _nthreads())
    return idx, d2


# --------------------------------------------------------------------------- neighbour lists
NEIGHBORS_MAX_K = 1024  # knn_neighbors.hip: a row's sort stays within 8 KB of LDS


def _walk_view(what: str, tree: tuple, qsorted: torch.Tensor, nq: int, out_perm: torch.Tensor) -> TreeView:
    """The view of `tree` for a group walk (ball_walk.h) by `what`, whose curve-sorted queries
    and sorted query -> query row map are checked."""
    pts, nodes, qnodes, n, depth = tree
    if qsorted.shape[0] < nq or out_perm.dtype != torch.int32 or out_perm.numel() < nq \
            or not out_perm.is_contiguous() or out_perm.device != pts.device or qsorted.device != pts.device:
        raise ValueError(f"{what}: qsorted [>= nq, 3] and out_perm int32 [nq], contiguous, on the tree's device")
    return TreeView(_ptr(pts), _ptr(nodes), _ptr(qnodes), n, depth, 0)


def knn_neighbors_gpu(tree: tuple, perm: torch.Tensor, qsorted: torch.Tensor, nq: int, kth_d2: torch.Tensor,
                      k: int, cut2: float, out_perm: torch.Tensor, out_idx: torch.Tensor,
                      out_dist: torch.Tensor) -> torch.Tensor:
    """The collect pass of the neighbour lists (knn_neighbors.hip) on the current stream:
    fills out_idx (int32 [nq, k]) / out_dist (float32 [nq, k]) in query order from the
    curve-sorted queries' exact k-th squared distances `kth_d2`. tree: (sorted_pts_padded,
    nodes, qnodes, n, depth), unrotated, n >= 1. Returns the pass's device error word (int32
    [1]; non-zero: kth_d2 was not the k-th value of some query, the caller raises)."""
    if not 1 <= k <= NEIGHBORS_MAX_K:
        raise ValueError(f"knn_neighbors_gpu: k must be in [1, {NEIGHBORS_MAX_K}]")
    tv = _walk_view("knn_neighbors_gpu", tree, qsorted, nq, out_perm)
    pts = tree[0]
    for t, dt, cnt in ((perm, torch.int32, tree[3]), (kth_d2, torch.float32, nq),
                       (out_idx, torch.int32, nq * k), (out_dist, torch.float32, nq * k)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() < cnt or t.device != pts.device:
            raise ValueError("knn_neighbors_gpu: perm int32, kth_d2 / out_dist float32, out_idx int32, "
                             "contiguous, on the tree's device and large enough")
    if out_idx.numel() != nq * k or out_dist.numel() != nq * k:
        raise ValueError("knn_neighbors_gpu: outputs must be [nq, k]")
    lib = _native.hip()
    err = torch.zeros(1, dtype=torch.int32, device=pts.device)
    ws = torch.empty(int(lib.lsk_hip_knn_neighbors_ws_bytes(int(nq))) // 4, dtype=torch.int32, device=pts.device)
    check(lib.lsk_hip_knn_neighbors(C.byref(tv), _ptr(perm), _ptr(qsorted), _ptr(kth_d2), int(nq), int(k),
                                    C.c_float(cut2), _ptr(out_perm), _ptr(out_idx), _ptr(out_dist), _ptr(err),
                                    _ptr(ws), _stream(pts)), "knn_neighbors")
    return err


# --------------------------------------------------------------------------- fixed-radius search
RADIUS_LDS_ROW = 4096  # radius.hip kLdsRow: longer rows are sorted in global memory


def radius_count_cpu(points: torch.Tensor, queries: torch.Tensor, cut2: float) -> torch.Tensor:
    """CPU oracle (brute force): int32 [nq], per query the number of rows of `points` with
    dist2 < cut2 (strict)."""
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    counts = torch.empty(q.shape[0], dtype=torch.int32)
    _native.host().lsk_cpu_radius_count(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], C.c_float(cut2),
                                        _ptr(counts), _nthreads())
    return counts


def radius_cpu(points: torch.Tensor, queries: torch.Tensor, cut2: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CPU oracle of the fixed-radius lists (brute force), CSR: (offsets int64 [nq + 1], idx
    int32 [total], d2 float32 [total]); row q holds every (row of `points`, dist2) with
    dist2 < cut2 in ascending (dist2 bits, row) order."""
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    nq = q.shape[0]
    offsets = torch.zeros(nq + 1, dtype=torch.int64)
    torch.cumsum(radius_count_cpu(pts, q, cut2), 0, dtype=torch.int64, out=offsets[1:])
    total = int(offsets[nq])
    idx = torch.empty(total, dtype=torch.int32)
    d2 = torch.empty(total, dtype=torch.float32)
    _native.host().lsk_cpu_radius_fill(_ptr(pts), pts.shape[0], _ptr(q), nq, C.c_float(cut2), _ptr(offsets),
                                       _ptr(idx), _ptr(d2), _nthreads())
    return offsets, idx, d2


def _var_cut2_cpu(what: str, cut2: torch.Tensor | None, count: int) -> torch.Tensor | None:
    if cut2 is None:
        return None
    c = cut2.contiguous().float().cpu()
    if c.shape != (count,):
        raise ValueError(f"{what}: {tuple(c.shape)} cutoffs for {count} rows")
    return c


def radius_var_count_cpu(points: torch.Tensor, queries: torch.Tensor, qcut2: torch.Tensor | None = None,
                         pcut2: torch.Tensor | None = None) -> torch.Tensor:
    """CPU oracle (brute force) of the variable-radius counts: int32 [nq], per query q the
    number of rows p of `points` with dist2 < qcut2[q] (float32 [nq], when given) and dist2 <
    pcut2[p] (float32 [n], in the order of `points`, when given); strict."""
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    qc = _var_cut2_cpu("radius_var_count_cpu", qcut2, q.shape[0])
    pc = _var_cut2_cpu("radius_var_count_cpu", pcut2, pts.shape[0])
    counts = torch.empty(q.shape[0], dtype=torch.int32)
    _native.host().lsk_cpu_radius_var_count(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], _ptr(qc), _ptr(pc),
                                            _ptr(counts), _nthreads())
    return counts


def radius_var_cpu(points: torch.Tensor, queries: torch.Tensor, qcut2: torch.Tensor | None = None,
                   pcut2: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CPU oracle of the variable-radius lists (brute force), the CSR form and row order of
    radius_cpu under the predicate of radius_var_count_cpu."""
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    qc = _var_cut2_cpu("radius_var_cpu", qcut2, q.shape[0])
    pc = _var_cut2_cpu("radius_var_cpu", pcut2, pts.shape[0])
    nq = q.shape[0]
    offsets = torch.zeros(nq + 1, dtype=torch.int64)
    torch.cumsum(radius_var_count_cpu(pts, q, qc, pc), 0, dtype=torch.int64, out=offsets[1:])
    total = int(offsets[nq])
    idx = torch.empty(total, dtype=torch.int32)
    d2 = torch.empty(total, dtype=torch.float32)
    _native.host().lsk_cpu_radius_var_fill(_ptr(pts), pts.shape[0], _ptr(q), nq, _ptr(qc), _ptr(pc), _ptr(offsets),
                                           _ptr(idx), _ptr(d2), _nthreads())
    return offsets, idx, d2


def _radius_var_args(what: str, tree: tuple, qsorted: torch.Tensor, nq: int, out_perm: torch.Tensor,
                     qcut2: torch.Tensor | None, pcut2: torch.Tensor | None):
    if (qcut2 is None) == (pcut2 is None):
        raise ValueError(f"{what}: exactly one of qcut2 and pcut2")
    t, cnt = (qcut2, nq) if qcut2 is not None else (pcut2, tree[3])
    if t.dtype != torch.float32 or t.shape != (cnt,) or not t.is_contiguous() or t.device != tree[0].device:
        raise ValueError(f"{what}: cutoffs float32 [{cnt}], contiguous, on the tree's device")
    return _walk_view(what, tree, qsorted, nq, out_perm)


def radius_var_count_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, out_perm: torch.Tensor,
                         qcut2: torch.Tensor | None = None, pcut2: torch.Tensor | None = None,
                         stats: torch.Tensor | None = None) -> torch.Tensor:
    """The count pass of the variable-radius search (radius_var.hip), as radius_count_gpu.
    qcut2: float32 [nq] squared cutoffs in query order (gather), or pcut2: float32 [n] in the
    order of the tree's sorted points (scatter), the tree's node array then being a copy
    annotated with them (tree_set_radii). Entries >= 0, no NaN: the caller checks."""
    tv = _radius_var_args("radius_var_count_gpu", tree, qsorted, nq, out_perm, qcut2, pcut2)
    counts = torch.empty(nq, dtype=torch.int32, device=tree[0].device)
    check(_native.hip().lsk_hip_radius_var_count(C.byref(tv), _ptr(qsorted), int(nq), _ptr(qcut2), _ptr(pcut2),
                                                 _ptr(out_perm), _ptr(counts), _ptr(stats), _stream(tree[0])),
          "radius_var_count")
    return counts


def radius_var_fill_gpu(tree: tuple, perm: torch.Tensor, qsorted: torch.Tensor, nq: int, out_perm: torch.Tensor,
                        offsets: torch.Tensor, total: int, longest: int, qcut2: torch.Tensor | None = None,
                        pcut2: torch.Tensor | None = None,
                        sort: bool = True) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fill and sort passes of the variable-radius search, as radius_fill_gpu (the sort
    is lsk_hip_radius_sort itself); cutoffs as for radius_var_count_gpu."""
    tv = _radius_var_args("radius_var_fill_gpu", tree, qsorted, nq, out_perm, qcut2, pcut2)
    dev = tree[0].device
    if offsets.dtype != torch.int64 or offsets.numel() != nq + 1 or not offsets.is_contiguous() or offsets.device != dev \
            or perm.dtype != torch.int32 or perm.numel() < tree[3] or not perm.is_contiguous() or perm.device != dev:
        raise ValueError("radius_var_fill_gpu: offsets int64 [nq + 1] and perm int32 [n], contiguous, on the tree's device")
    lib = _native.hip()
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    dist = torch.empty(total, dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.lsk_hip_radius_var_fill(C.byref(tv), _ptr(perm), _ptr(qsorted), int(nq), _ptr(qcut2), _ptr(pcut2),
                                      _ptr(out_perm), _ptr(offsets), _ptr(idx), _ptr(dist), _ptr(err),
                                      _stream(tree[0])), "radius_var_fill")
    check(lib.lsk_hip_radius_sort(_ptr(offsets), int(nq), int(total), int(longest), _ptr(idx), _ptr(dist),
                                  1 if sort else 0, _stream(tree[0])), "radius_sort")
    return idx, dist, err


def _radius_args(what: str, tree: tuple, qsorted: torch.Tensor, nq: int, cut2: float, out_perm: torch.Tensor):
    if not cut2 >= 0.0:
        raise ValueError(f"{what}: cut2 must be >= 0")
    return _walk_view(what, tree, qsorted, nq, out_perm)


def radius_count_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, cut2: float, out_perm: torch.Tensor,
                     stats: torch.Tensor | None = None) -> torch.Tensor:
    """The count pass of the fixed-radius search (radius.hip) on the current stream: int32
    [nq] in query order, per query the number of the tree's points with dist2 < cut2. tree:
    (sorted_pts_padded, nodes, qnodes, n, depth), unrotated, n >= 1; qsorted / out_perm: the
    curve-sorted queries and sorted query -> query row. stats: optional zeroed int64 [4]
    (distance evaluations, nodes popped, buckets scanned, whole-box acceptances)."""
    tv = _radius_args("radius_count_gpu", tree, qsorted, nq, cut2, out_perm)
    counts = torch.empty(nq, dtype=torch.int32, device=tree[0].device)
    check(_native.hip().lsk_hip_radius_count(C.byref(tv), _ptr(qsorted), int(nq), C.c_float(cut2), _ptr(out_perm),
                                             _ptr(counts), _ptr(stats), _stream(tree[0])), "radius_count")
    return counts


def radius_fill_gpu(tree: tuple, perm: torch.Tensor, qsorted: torch.Tensor, nq: int, cut2: float,
                    out_perm: torch.Tensor, offsets: torch.Tensor, total: int, longest: int,
                    sort: bool = True) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fill and sort passes of the fixed-radius search on the current stream: (idx int32
    [total], dist float32 [total], err) for the CSR rows `offsets` (int64 [nq + 1] on the
    device, the prefix sum of radius_count_gpu's counts for the same cut2; total =
    offsets[nq], longest >= the longest row). idx holds rows of the indexed array (through
    perm), dist final distances; sort: rows ascending by (dist2 bits, row), else in walk
    order. err: the device error word (int32 [1]; non-zero: count and fill disagreed, the
    caller raises)."""
    tv = _radius_args("radius_fill_gpu", tree, qsorted, nq, cut2, out_perm)
    dev = tree[0].device
    if offsets.dtype != torch.int64 or offsets.numel() != nq + 1 or not offsets.is_contiguous() or offsets.device != dev \
            or perm.dtype != torch.int32 or perm.numel() < tree[3] or not perm.is_contiguous() or perm.device != dev:
        raise ValueError("radius_fill_gpu: offsets int64 [nq + 1] and perm int32 [n], contiguous, on the tree's device")
    lib = _native.hip()
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    dist = torch.empty(total, dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.lsk_hip_radius_fill(C.byref(tv), _ptr(perm), _ptr(qsorted), int(nq), C.c_float(cut2), _ptr(out_perm),
                                  _ptr(offsets), _ptr(idx), _ptr(dist), _ptr(err), _stream(tree[0])), "radius_fill")
    check(lib.lsk_hip_radius_sort(_ptr(offsets), int(nq), int(total), int(longest), _ptr(idx), _ptr(dist),
                                  1 if sort else 0, _stream(tree[0])), "radius_sort")
    return idx, dist, err


# --------------------------------------------------------------------------- density clustering
def cluster_cpu(points: torch.Tensor, cut2: float, min_pts: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
    """CPU oracle of the density clustering (brute force over all pairs): (labels int32 [n],
    core bool [n]) in the order of `points`. core: at least min_pts points (itself and exact
    copies included) with dist2 < cut2 (strict); a core point's label is the smallest row among
    the core points of its connected component, a non-core point's the label of its nearest
    core point by (dist2 bits, row) within cut2, else -1 (min_pts = 1: its own row)."""
    if min_pts < 1 or not cut2 >= 0.0:
        raise ValueError("cluster_cpu: min_pts must be at least 1 and cut2 >= 0")
    pts = points.contiguous().float().cpu()
    n = pts.shape[0]
    labels = torch.empty(n, dtype=torch.int32)
    core = torch.empty(n, dtype=torch.uint8)
    _native.host().lsk_cpu_cluster(_ptr(pts), n, C.c_float(cut2), int(min_pts), _ptr(labels), _ptr(core), _nthreads())
    return labels, core.bool()


CLUSTER_STATS = 5  # cluster.hip: distance evaluations, nodes popped, buckets scanned, clique acceptances, CAS retries


def cluster_gpu(tree: tuple, perm: torch.Tensor, core_sorted: torch.Tensor, cut2: float, fof: bool,
                border: bool, half: bool = False, stats: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """The passes of the density clustering (cluster.hip) on the current stream: (labels int32
    [n] in input order, err: the device error word, int32 [1]; non-zero: a parent chain did not
    end, the caller raises). tree: (sorted_pts_padded, nodes, qnodes, n, depth), unrotated, n
    >= 1; perm: sorted position -> input row; core_sorted: uint8 [n], the core flags at the
    sorted positions. fof: a non-core point is a cluster of its own (min_pts = 1), else noise;
    border: also run the border walk (non-core points take their nearest core point's label).
    half: see lsk_hip_cluster_link. stats: optional zeroed int64 [CLUSTER_STATS]."""
    pts, nodes, qnodes, n, depth = tree
    dev = pts.device
    if not cut2 >= 0.0:
        raise ValueError("cluster_gpu: cut2 must be >= 0")
    for t, dt in ((perm, torch.int32), (core_sorted, torch.uint8)):
        if t.dtype != dt or t.numel() < n or not t.is_contiguous() or t.device != dev:
            raise ValueError("cluster_gpu: perm int32 [n] and core_sorted uint8 [n], contiguous, on the tree's device")
    if stats is not None and (stats.dtype != torch.int64 or stats.numel() < CLUSTER_STATS or stats.device != dev):
        raise ValueError(f"cluster_gpu: stats int64 [{CLUSTER_STATS}] on the tree's device")
    tv = TreeView(_ptr(pts), _ptr(nodes), _ptr(qnodes), n, depth, 0)
    cpre = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    torch.cumsum(core_sorted[:n], 0, dtype=torch.int32, out=cpre[1:])
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    root = torch.empty(n, dtype=torch.int32, device=dev)
    minrow = torch.empty(n, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    lib, st = _native.hip(), _stream(pts)
    check(lib.lsk_hip_cluster_link(C.byref(tv), _ptr(core_sorted), _ptr(cpre), C.c_float(cut2), 1 if half else 0,
                                   _ptr(parent), _ptr(minrow), _ptr(err), _ptr(stats), st), "cluster_link")
    check(lib.lsk_hip_cluster_label(C.byref(tv), _ptr(perm), _ptr(core_sorted), _ptr(parent), 1 if fof else 0,
                                    _ptr(root), _ptr(minrow), _ptr(labels), _ptr(err), st), "cluster_label")
    if border:
        check(lib.lsk_hip_cluster_border(C.byref(tv), _ptr(perm), _ptr(core_sorted), C.c_float(cut2), _ptr(root),
                                         _ptr(minrow), _ptr(labels), _ptr(stats), st), "cluster_border")
    return labels, err


# --------------------------------------------------------------------------- minimum spanning tree
def mst_cpu(points: torch.Tensor, core_d2: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """CPU oracle of the Euclidean minimum spanning tree (Prim over all pairs): (rows int32 [m,
    2], d2 float32 [m]). Vertices are the points with finite coordinates, m = max(their number -
    1, 0); the weight of {a, b} is w = dist2(a, b), with core_d2 (float32 [n], every entry finite
    and >= 0) max(dist2(a, b), core_d2[a], core_d2[b]); edges are ordered by (bits of w, lo, hi)
    with lo < hi the two rows, a strict total order, so the tree is unique. Each row of `rows` is
    (lo, hi), d2 holds w, both ascending by that key."""
    pts = points.contiguous().float().cpu()
    n = pts.shape[0]
    core = None
    if core_d2 is not None:
        core = core_d2.contiguous().float().cpu()
        if core.dim() != 1 or core.shape[0] != n or not bool((torch.isfinite(core) & (core >= 0)).all()):
            raise ValueError("mst_cpu: core_d2 must hold n finite entries >= 0")
    rows = torch.empty((max(n - 1, 0), 2), dtype=torch.int32)
    d2 = torch.empty(max(n - 1, 0), dtype=torch.float32)
    m = int(_native.host().lsk_cpu_mst(_ptr(pts), n, _ptr(core), _ptr(rows), _ptr(d2)))
    return rows[:m].contiguous(), d2[:m].contiguous()


def mst_labels_cpu(rows: torch.Tensor, d2: torch.Tensor, n: int, cut2: float) -> torch.Tensor:
    """labels int32 [n]: the smallest row of every row's component under the edges with d2 < cut2."""
    rows = rows.contiguous()
    d2 = d2.contiguous()
    labels = torch.empty(n, dtype=torch.int32)
    if _native.host().lsk_cpu_mst_labels(_ptr(rows), _ptr(d2), d2.shape[0], C.c_float(cut2), n, _ptr(labels)):
        raise ValueError(f"mst_labels: an edge names a row outside [0, {n})")
    return labels


MST_STATS = 5  # mst.hip: distance evaluations, nodes popped, buckets scanned, image walks (periodic), CAS retries


class MstState:
    """The device buffers of the Boruvka rounds over one tree (mst.hip): O(n)."""

    def __init__(self, tree: tuple, perm: torch.Tensor, core_sorted: torch.Tensor | None,
                 stats: torch.Tensor | None = None, period: tuple[float, float, float] | None = None):
        """period: check_period's values (the periodic rounds), None: the open box."""
        pts, nodes, qnodes, n, depth = tree
        dev = pts.device
        if perm.dtype != torch.int32 or perm.numel() < n or not perm.is_contiguous() or perm.device != dev:
            raise ValueError("mst_gpu: perm int32 [n], contiguous, on the tree's device")
        if core_sorted is not None and (core_sorted.dtype != torch.float32 or core_sorted.numel() != n
                                        or not core_sorted.is_contiguous() or core_sorted.device != dev):
            raise ValueError("mst_gpu: core_sorted float32 [n], contiguous, on the tree's device")
        if stats is not None and (stats.dtype != torch.int64 or stats.numel() < MST_STATS or stats.device != dev):
            raise ValueError(f"mst_gpu: stats int64 [{MST_STATS}] on the tree's device")
        self.tv = TreeView(_ptr(pts), _ptr(nodes), _ptr(qnodes), n, depth, 0)
        self.keep = (pts, nodes, qnodes, perm, core_sorted, stats)  # (the view holds raw pointers)
        self.period = None if period is None else _period_c(period)
        self.n = n
        self.parent = torch.arange(n, dtype=torch.int32, device=dev)
        self.comp = torch.empty(n, dtype=torch.int32, device=dev)
        self.ncomp = torch.empty(2 << depth, dtype=torch.int32, device=dev)
        self.best = torch.empty(n, dtype=torch.int64, device=dev)
        self.best_pos = torch.empty(n, dtype=torch.int32, device=dev)
        self.cmin = torch.empty(n, dtype=torch.int64, device=dev)
        self.chi = torch.empty(n, dtype=torch.int32, device=dev)
        self.rows = torch.empty((n, 2), dtype=torch.int32, device=dev)
        self.d2 = torch.empty(n, dtype=torch.float32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)

    def round(self) -> None:
        """One Boruvka round on the current stream (no host read)."""
        pts, _, _, perm, core, stats = self.keep
        tail = (_ptr(self.parent), _ptr(self.comp), _ptr(self.ncomp), _ptr(self.best), _ptr(self.best_pos),
                _ptr(self.cmin), _ptr(self.chi), _ptr(self.rows), _ptr(self.d2), _ptr(self.count), _ptr(self.err),
                _ptr(stats), _stream(pts))
        if self.period is None:
            check(_native.hip().lsk_hip_mst_round(C.byref(self.tv), _ptr(perm), _ptr(core), *tail), "mst_round")
        else:
            check(_native.hip().lsk_hip_mst_periodic_round(C.byref(self.tv), _ptr(perm), _ptr(core), self.period,
                                                           *tail), "mst_periodic_round")


def mst_labels_gpu(rows: torch.Tensor, d2: torch.Tensor, n: int, cut2: float) -> tuple[torch.Tensor, torch.Tensor]:
    """(labels int32 [n], err int32 [1]) of device edges (rows int32 [m, 2], d2 float32 [m], n >=
    1): the edge hook of mst.hip, then the label passes of cluster.hip over the rows themselves
    (identity perm, every row a core point, a row without an edge its own label)."""
    dev = d2.device
    m = d2.shape[0]
    rows = rows.contiguous()
    d2 = d2.contiguous()
    lib, st = _native.hip(), _stream(d2)
    parent = torch.arange(n, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.lsk_hip_mst_cut(_ptr(rows), _ptr(d2), m, C.c_float(cut2), n, _ptr(parent), _ptr(err), st), "mst_cut")
    ident = torch.arange(n, dtype=torch.int32, device=dev)
    core = torch.ones(n, dtype=torch.uint8, device=dev)
    root = torch.empty(n, dtype=torch.int32, device=dev)
    minrow = torch.full((n,), -1, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    # the label passes read the view's n alone; its pointers only have to be non-null
    tv = TreeView(_ptr(ident), _ptr(ident), None, n, int(lib.lsk_hip_tree_depth(n)), 0)
    check(lib.lsk_hip_cluster_label(C.byref(tv), _ptr(ident), _ptr(core), _ptr(parent), 1, _ptr(root),
                                    _ptr(minrow), _ptr(labels), _ptr(err), st), "cluster_label")
    return labels, err


# --------------------------------------------------------------------------- periodic box
RADIUS_PERIODIC_STATS = 5  # periodic.hip: the four of radius.hip and the image walks


def check_period(what: str, period) -> tuple[float, float, float]:
    """(Lx, Ly, Lz) as float32 values: a scalar is broadcast; every entry > 0, inf = open axis.
    Anything else (NaN, <= 0, not one or three values) raises ValueError."""
    if isinstance(period, torch.Tensor):
        period = period.detach().cpu().tolist()
    if isinstance(period, (int, float)) and not isinstance(period, bool):
        period = (period,) * 3
    try:
        vals = tuple(float(torch.tensor(float(v), dtype=torch.float32)) for v in period)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: period must be one value or three (got {period!r})") from None
    if len(vals) != 3:
        raise ValueError(f"{what}: period must be one value or three (got {len(vals)})")
    if not all(v > 0.0 for v in vals):  # (a NaN fails the comparison too)
        raise ValueError(f"{what}: every period entry must be > 0 (inf: open axis), got {vals}")
    return vals


def period_cut2_bound(period: tuple[float, float, float]) -> float:
    """The largest squared cutoff a period admits: the smallest fl(h * h), h = fl(0.5 L), over its
    finite axes (inf when every axis is open), in float32 arithmetic."""
    L = torch.tensor(period, dtype=torch.float32)
    h = L * 0.5
    return float((h * h).min())


def _period_c(period: tuple[float, float, float]):
    return (C.c_float * 3)(*period)


def radius_periodic_count_cpu(points: torch.Tensor, queries: torch.Tensor, cut2: float, period,
                              qcut2: torch.Tensor | None = None) -> torch.Tensor:
    """CPU oracle (brute force) of the periodic counts: radius_count_cpu with dist2 replaced by the
    minimum image of the difference under `period` (per axis d = q - p; d > L/2: d - L; d <
    -L/2: d + L, in float32), strict. qcut2 (float32 [nq]) replaces cut2 per query."""
    per = check_period("radius_periodic_count_cpu", period)
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    qc = _var_cut2_cpu("radius_periodic_count_cpu", qcut2, q.shape[0])
    counts = torch.empty(q.shape[0], dtype=torch.int32)
    _native.host().lsk_cpu_radius_periodic_count(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], C.c_float(cut2),
                                                 _ptr(qc), _period_c(per), _ptr(counts), _nthreads())
    return counts


def radius_periodic_cpu(points: torch.Tensor, queries: torch.Tensor, cut2: float, period,
                        qcut2: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CPU oracle of the periodic radius lists, the CSR form and row order of radius_cpu under the
    predicate of radius_periodic_count_cpu (d2: the periodic squared distances)."""
    per = check_period("radius_periodic_cpu", period)
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    nq = q.shape[0]
    qc = _var_cut2_cpu("radius_periodic_cpu", qcut2, nq)
    offsets = torch.zeros(nq + 1, dtype=torch.int64)
    torch.cumsum(radius_periodic_count_cpu(pts, q, cut2, per, qc), 0, dtype=torch.int64, out=offsets[1:])
    total = int(offsets[nq])
    idx = torch.empty(total, dtype=torch.int32)
    d2 = torch.empty(total, dtype=torch.float32)
    _native.host().lsk_cpu_radius_periodic_fill(_ptr(pts), pts.shape[0], _ptr(q), nq, C.c_float(cut2), _ptr(qc),
                                                _period_c(per), _ptr(offsets), _ptr(idx), _ptr(d2), _nthreads())
    return offsets, idx, d2


def cluster_periodic_cpu(points: torch.Tensor, cut2: float, min_pts: int = 1,
                         period=math.inf) -> tuple[torch.Tensor, torch.Tensor]:
    """CPU oracle of the periodic density clustering: cluster_cpu with the periodic squared
    distance of radius_periodic_count_cpu."""
    if min_pts < 1 or not cut2 >= 0.0:
        raise ValueError("cluster_periodic_cpu: min_pts must be at least 1 and cut2 >= 0")
    per = check_period("cluster_periodic_cpu", period)
    pts = points.contiguous().float().cpu()
    n = pts.shape[0]
    labels = torch.empty(n, dtype=torch.int32)
    core = torch.empty(n, dtype=torch.uint8)
    _native.host().lsk_cpu_cluster_periodic(_ptr(pts), n, C.c_float(cut2), int(min_pts), _period_c(per),
                                            _ptr(labels), _ptr(core), _nthreads())
    return labels, core.bool()


def _periodic_view(what: str, tree: tuple, qsorted: torch.Tensor, nq: int, out_perm: torch.Tensor,
                   cut2: float, qcut2: torch.Tensor | None):
    if qcut2 is None:
        if not cut2 >= 0.0:
            raise ValueError(f"{what}: cut2 must be >= 0")
    elif qcut2.dtype != torch.float32 or qcut2.shape != (nq,) or not qcut2.is_contiguous() \
            or qcut2.device != tree[0].device:
        raise ValueError(f"{what}: qcut2 float32 [{nq}], contiguous, on the tree's device")
    return _walk_view(what, tree, qsorted, nq, out_perm)


def radius_periodic_count_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, cut2: float, out_perm: torch.Tensor,
                              period: tuple[float, float, float], qcut2: torch.Tensor | None = None,
                              stats: torch.Tensor | None = None) -> torch.Tensor:
    """The count pass of the periodic radius search (periodic.hip), as radius_count_gpu. period:
    check_period's values; qcut2: float32 [nq] squared cutoffs in query order in place of cut2
    (entries >= 0, no NaN, within the period's bound: the caller checks). stats: optional zeroed
    int64 [RADIUS_PERIODIC_STATS]."""
    tv = _periodic_view("radius_periodic_count_gpu", tree, qsorted, nq, out_perm, cut2, qcut2)
    counts = torch.empty(nq, dtype=torch.int32, device=tree[0].device)
    check(_native.hip().lsk_hip_radius_periodic_count(C.byref(tv), _ptr(qsorted), int(nq), C.c_float(cut2),
                                                      _ptr(qcut2), _period_c(period), _ptr(out_perm), _ptr(counts),
                                                      _ptr(stats), _stream(tree[0])), "radius_periodic_count")
    return counts


def radius_periodic_fill_gpu(tree: tuple, perm: torch.Tensor, qsorted: torch.Tensor, nq: int, cut2: float,
                             out_perm: torch.Tensor, offsets: torch.Tensor, total: int, longest: int,
                             period: tuple[float, float, float], qcut2: torch.Tensor | None = None,
                             sort: bool = True) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fill and sort passes of the periodic radius search, as radius_fill_gpu (the sort is
    lsk_hip_radius_sort itself); period / qcut2 as for radius_periodic_count_gpu."""
    tv = _periodic_view("radius_periodic_fill_gpu", tree, qsorted, nq, out_perm, cut2, qcut2)
    dev = tree[0].device
    if offsets.dtype != torch.int64 or offsets.numel() != nq + 1 or not offsets.is_contiguous() or offsets.device != dev \
            or perm.dtype != torch.int32 or perm.numel() < tree[3] or not perm.is_contiguous() or perm.device != dev:
        raise ValueError("radius_periodic_fill_gpu: offsets int64 [nq + 1] and perm int32 [n], contiguous, "
                         "on the tree's device")
    lib = _native.hip()
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    dist = torch.empty(total, dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.lsk_hip_radius_periodic_fill(C.byref(tv), _ptr(perm), _ptr(qsorted), int(nq), C.c_float(cut2),
                                           _ptr(qcut2), _period_c(period), _ptr(out_perm), _ptr(offsets), _ptr(idx),
                                           _ptr(dist), _ptr(err), _stream(tree[0])), "radius_periodic_fill")
    check(lib.lsk_hip_radius_sort(_ptr(offsets), int(nq), int(total), int(longest), _ptr(idx), _ptr(dist),
                                  1 if sort else 0, _stream(tree[0])), "radius_sort")
    return idx, dist, err


# ---- two-sided radii: a cutoff per query and per point (radius_reach.hip)
REACH_RULES = {"either": 0, "both": 1}  # LSK_REACH_EITHER / LSK_REACH_BOTH


def reach_rule(what: str, rule) -> int:
    """The native code of rule "either" (d2 < max(cq, cp)) or "both" (d2 < min(cq, cp));
    anything else raises ValueError."""
    if not isinstance(rule, str) or rule not in REACH_RULES:
        raise ValueError(f"{what}: rule must be 'either' or 'both' (got {rule!r})")
    return REACH_RULES[rule]


def _reach_cpu_args(what: str, points, queries, qcut2, pcut2, rule, period):
    code = reach_rule(what, rule)
    per = None if period is None else check_period(what, period)
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    qc = _var_cut2_cpu(what, qcut2, q.shape[0])
    pc = _var_cut2_cpu(what, pcut2, pts.shape[0])
    if qc is None or pc is None:
        raise ValueError(f"{what}: both qcut2 and pcut2 are required")
    return pts, q, qc, pc, code, None if per is None else _period_c(per)


def radius_reach_count_cpu(points: torch.Tensor, queries: torch.Tensor, qcut2: torch.Tensor, pcut2: torch.Tensor,
                           rule: str = "either", period=None) -> torch.Tensor:
    """CPU oracle (brute force) of the two-sided radius counts: int32 [nq], per query q the number
    of rows p of `points` with d2 < max(qcut2[q], pcut2[p]) (rule "either") or d2 < min(qcut2[q],
    pcut2[p]) ("both"), strict; qcut2 float32 [nq], pcut2 float32 [n] in the order of `points`.
    d2 is dist2, or under `period` the minimum image of radius_periodic_count_cpu."""
    pts, q, qc, pc, code, per = _reach_cpu_args("radius_reach_count_cpu", points, queries, qcut2, pcut2, rule, period)
    counts = torch.empty(q.shape[0], dtype=torch.int32)
    _native.host().lsk_cpu_radius_reach_count(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], _ptr(qc), _ptr(pc), code,
                                              per, _ptr(counts), _nthreads())
    return counts


def radius_reach_cpu(points: torch.Tensor, queries: torch.Tensor, qcut2: torch.Tensor, pcut2: torch.Tensor,
                     rule: str = "either", period=None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CPU oracle of the two-sided radius lists (brute force), the CSR form and row order of
    radius_cpu under the predicate of radius_reach_count_cpu."""
    pts, q, qc, pc, code, per = _reach_cpu_args("radius_reach_cpu", points, queries, qcut2, pcut2, rule, period)
    nq = q.shape[0]
    counts = torch.empty(nq, dtype=torch.int32)
    lib = _native.host()
    lib.lsk_cpu_radius_reach_count(_ptr(pts), pts.shape[0], _ptr(q), nq, _ptr(qc), _ptr(pc), code, per,
                                   _ptr(counts), _nthreads())
    offsets = torch.zeros(nq + 1, dtype=torch.int64)
    torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    total = int(offsets[nq])
    idx = torch.empty(total, dtype=torch.int32)
    d2 = torch.empty(total, dtype=torch.float32)
    lib.lsk_cpu_radius_reach_fill(_ptr(pts), pts.shape[0], _ptr(q), nq, _ptr(qc), _ptr(pc), code, per,
                                  _ptr(offsets), _ptr(idx), _ptr(d2), _nthreads())
    return offsets, idx, d2


def _reach_view(what: str, tree: tuple, qsorted: torch.Tensor, nq: int, out_perm: torch.Tensor,
                qcut2: torch.Tensor, pcut2: torch.Tensor):
    dev = tree[0].device
    for t, cnt, nm in ((qcut2, nq, "qcut2"), (pcut2, tree[3], "pcut2")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.shape != (cnt,) \
                or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{what}: {nm} float32 [{cnt}], contiguous, on the tree's device")
    return _walk_view(what, tree, qsorted, nq, out_perm)


def radius_reach_count_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, out_perm: torch.Tensor, qcut2: torch.Tensor,
                           pcut2: torch.Tensor, rule: str, period: tuple[float, float, float] | None = None,
                           stats: torch.Tensor | None = None) -> torch.Tensor:
    """The count pass of the two-sided radius search (radius_reach.hip), as radius_count_gpu.
    qcut2: float32 [nq] squared cutoffs in query order; pcut2: float32 [n] in the order of the
    tree's sorted points, the tree's node array being a copy annotated with them
    (tree_set_radii). Entries >= 0, no NaN, within the period's bound: the caller checks. period:
    check_period's values, or None for the open box (the walk without an image loop). stats:
    optional zeroed int64 [4] (period: [RADIUS_PERIODIC_STATS])."""
    code = reach_rule("radius_reach_count_gpu", rule)
    tv = _reach_view("radius_reach_count_gpu", tree, qsorted, nq, out_perm, qcut2, pcut2)
    counts = torch.empty(nq, dtype=torch.int32, device=tree[0].device)
    check(_native.hip().lsk_hip_radius_reach_count(C.byref(tv), _ptr(qsorted), int(nq), _ptr(qcut2), _ptr(pcut2),
                                                   code, None if period is None else _period_c(period),
                                                   _ptr(out_perm), _ptr(counts), _ptr(stats), _stream(tree[0])),
          "radius_reach_count")
    return counts


def radius_reach_fill_gpu(tree: tuple, perm: torch.Tensor, qsorted: torch.Tensor, nq: int, out_perm: torch.Tensor,
                          offsets: torch.Tensor, total: int, longest: int, qcut2: torch.Tensor, pcut2: torch.Tensor,
                          rule: str, period: tuple[float, float, float] | None = None,
                          sort: bool = True) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fill and sort passes of the two-sided radius search, as radius_fill_gpu (the sort is
    lsk_hip_radius_sort itself); cutoffs, rule and period as for radius_reach_count_gpu."""
    code = reach_rule("radius_reach_fill_gpu", rule)
    tv = _reach_view("radius_reach_fill_gpu", tree, qsorted, nq, out_perm, qcut2, pcut2)
    dev = tree[0].device
    if offsets.dtype != torch.int64 or offsets.numel() != nq + 1 or not offsets.is_contiguous() or offsets.device != dev \
            or perm.dtype != torch.int32 or perm.numel() < tree[3] or not perm.is_contiguous() or perm.device != dev:
        raise ValueError("radius_reach_fill_gpu: offsets int64 [nq + 1] and perm int32 [n], contiguous, "
                         "on the tree's device")
    lib = _native.hip()
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    dist = torch.empty(total, dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.lsk_hip_radius_reach_fill(C.byref(tv), _ptr(perm), _ptr(qsorted), int(nq), _ptr(qcut2), _ptr(pcut2),
                                        code, None if period is None else _period_c(period), _ptr(out_perm),
                                        _ptr(offsets), _ptr(idx), _ptr(dist), _ptr(err), _stream(tree[0])),
          "radius_reach_fill")
    check(lib.lsk_hip_radius_sort(_ptr(offsets), int(nq), int(total), int(longest), _ptr(idx), _ptr(dist),
                                  1 if sort else 0, _stream(tree[0])), "radius_sort")
    return idx, dist, err


def cluster_periodic_gpu(tree: tuple, perm: torch.Tensor, core_sorted: torch.Tensor, cut2: float,
                         period: tuple[float, float, float], fof: bool, border: bool, half: bool = False,
                         stats: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """cluster_gpu under a period: the init, flatten, min-row and label passes of cluster.hip
    around the periodic hook and border walks of periodic.hip. core_sorted comes from the
    periodic count."""
    pts, nodes, qnodes, n, depth = tree
    dev = pts.device
    if not cut2 >= 0.0:
        raise ValueError("cluster_periodic_gpu: cut2 must be >= 0")
    for t, dt in ((perm, torch.int32), (core_sorted, torch.uint8)):
        if t.dtype != dt or t.numel() < n or not t.is_contiguous() or t.device != dev:
            raise ValueError("cluster_periodic_gpu: perm int32 [n] and core_sorted uint8 [n], contiguous, "
                             "on the tree's device")
    if stats is not None and (stats.dtype != torch.int64 or stats.numel() < CLUSTER_STATS or stats.device != dev):
        raise ValueError(f"cluster_periodic_gpu: stats int64 [{CLUSTER_STATS}] on the tree's device")
    tv = TreeView(_ptr(pts), _ptr(nodes), _ptr(qnodes), n, depth, 0)
    cpre = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    torch.cumsum(core_sorted[:n], 0, dtype=torch.int32, out=cpre[1:])
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    root = torch.empty(n, dtype=torch.int32, device=dev)
    minrow = torch.empty(n, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    lib, st, per = _native.hip(), _stream(pts), _period_c(period)
    check(lib.lsk_hip_cluster_init(C.byref(tv), _ptr(core_sorted), _ptr(cpre), C.c_float(cut2), _ptr(parent),
                                   _ptr(minrow), st), "cluster_init")
    check(lib.lsk_hip_cluster_periodic_hook(C.byref(tv), _ptr(core_sorted), _ptr(cpre), C.c_float(cut2), per,
                                            1 if half else 0, _ptr(parent), _ptr(err), _ptr(stats), st),
          "cluster_periodic_hook")
    check(lib.lsk_hip_cluster_label(C.byref(tv), _ptr(perm), _ptr(core_sorted), _ptr(parent), 1 if fof else 0,
                                    _ptr(root), _ptr(minrow), _ptr(labels), _ptr(err), st), "cluster_label")
    if border:
        check(lib.lsk_hip_cluster_periodic_border(C.byref(tv), _ptr(perm), _ptr(core_sorted), C.c_float(cut2), per,
                                                  _ptr(root), _ptr(minrow), _ptr(labels), _ptr(stats), st),
              "cluster_periodic_border")
    return labels, err


# --------------------------------------------------------------------------- radius profiles
PROFILE_BINS = 32  # radius_profile.hip CountPolicy::kBins: cutoffs per launch, longer lists go in slices


def _profile_cut2s(what: str, cut2s) -> torch.Tensor:
    """The ascending squared cutoffs of a profile as a float32 CPU tensor [B], B >= 1."""
    c = torch.as_tensor(cut2s, dtype=torch.float32, device="cpu").contiguous()
    if c.dim() != 1 or c.shape[0] < 1:
        raise ValueError(f"{what}: cut2s must hold at least one cutoff (got shape {tuple(c.shape)})")
    if not bool((c >= 0).all()) or not bool((c[1:] >= c[:-1]).all()):  # (a NaN fails both)
        raise ValueError(f"{what}: cut2s must be >= 0, not NaN and ascending")
    return c


def radius_profile_cpu(points: torch.Tensor, queries: torch.Tensor, cut2s, period=None) -> torch.Tensor:
    """CPU oracle (brute force, one pass over the points per query): int32 [nq, B], column b =
    the number of rows of `points` with dist2 < cut2s[b] (strict), i.e. radius_count_cpu at that
    cutoff; with `period`, radius_periodic_count_cpu at that cutoff. cut2s: B >= 1 ascending
    squared cutoffs (a sequence or a CPU tensor)."""
    c = _profile_cut2s("radius_profile_cpu", cut2s)
    per = None if period is None else check_period("radius_profile_cpu", period)
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    out = torch.empty((q.shape[0], c.shape[0]), dtype=torch.int32)
    _native.host().lsk_cpu_radius_profile(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], _ptr(c), c.shape[0],
                                          None if per is None else _period_c(per), _ptr(out), _nthreads())
    return out


def pair_counts_cpu(points: torch.Tensor, queries: torch.Tensor, cut2s, period=None) -> torch.Tensor:
    """CPU oracle of the pair counts: int64 [B], the column sums of radius_profile_cpu."""
    return radius_profile_cpu(points, queries, cut2s, period).sum(0, dtype=torch.int64)


def _profile_stats(what: str, stats: torch.Tensor | None, period, dev: torch.device) -> None:
    need = RADIUS_PERIODIC_STATS if period is not None else 4
    if stats is not None and (stats.dtype != torch.int64 or stats.numel() < need or stats.device != dev):
        raise ValueError(f"{what}: stats int64 [{need}] on the tree's device")


def _query_weights_arg(what: str, wq: torch.Tensor | None, nq: int, dev: torch.device) -> torch.Tensor | None:
    if wq is not None and (wq.dtype != torch.int64 or wq.dim() != 1 or wq.shape[0] != nq or not wq.is_contiguous()
                           or wq.device != dev):
        raise ValueError(f"{what}: query_weights must be a contiguous int64 [{nq}] tensor on the tree's device")
    return wq


def _profile_slices(name: str, tree: tuple, qsorted: torch.Tensor, nq: int, cut2s, out_perm: torch.Tensor, period,
                    stats: torch.Tensor | None, sums: bool, weights: tuple | None = None,
                    query_weights: torch.Tensor | None = None) -> torch.Tensor:
    """What the four profile wrappers share: the argument checks, the result, and one call of
    lsk_hip_<name> per slice of cutoffs. sums: the [B] sums over the queries (with their block
    workspace) instead of the [nq, B] profile; weights: (wsorted, wpre) of the weighted forms."""
    what = name + "_gpu"
    c = _profile_cut2s(what, cut2s)
    tv = _walk_view(what, tree, qsorted, nq, out_perm)
    dev = tree[0].device
    _profile_stats(what, stats, period, dev)
    if weights is not None:
        _weighted_args(what, tree, *weights)
    wq = _query_weights_arg(what, query_weights, nq, dev)
    nb = c.shape[0]
    lib = _native.hip()
    if sums:
        res = torch.zeros(nb, dtype=torch.int64, device=dev)
        ws = torch.empty(int(getattr(lib, f"lsk_hip_{name}_ws_bytes")(int(nq))) // 8, dtype=torch.int64, device=dev)
        tail = (_ptr(ws), _ptr(res)) if weights is None else (_ptr(wq), _ptr(ws), _ptr(res))
    else:
        res = torch.empty((nq, nb), dtype=torch.int32 if weights is None else torch.int64, device=dev)
        tail = (_ptr(res), nb)
    cdev = c.to(dev)
    per = None if period is None else _period_c(period)
    fn = getattr(lib, "lsk_hip_" + name)
    width = PROFILE_BINS if weights is None else int(lib.lsk_hip_weighted_profile_bins())
    for col0 in range(0, nb, width):
        m = min(width, nb - col0)
        check(fn(C.byref(tv), _ptr(qsorted), int(nq), cdev.data_ptr() + 4 * col0, m, per, _ptr(out_perm),
                 *(_ptr(t) for t in weights or ()), *tail, col0, _ptr(stats), _stream(tree[0])), name)
    return res


def radius_profile_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, cut2s, out_perm: torch.Tensor,
                       period: tuple[float, float, float] | None = None,
                       stats: torch.Tensor | None = None) -> torch.Tensor:
    """The radius profile (radius_profile.hip) on the current stream: int32 [nq, B] in query
    order, column b = radius_count_gpu (period: radius_periodic_count_gpu) at cut2s[b], from one
    walk per slice of up to PROFILE_BINS cutoffs; every slice writes its own columns of the
    result. tree / qsorted / out_perm as for radius_count_gpu; cut2s: B >= 1 ascending squared
    cutoffs on the host (within the period's bound: the caller checks). stats: optional zeroed
    int64 [4] (period: [RADIUS_PERIODIC_STATS]), summed over the slices."""
    return _profile_slices("radius_profile", tree, qsorted, nq, cut2s, out_perm, period, stats, sums=False)


def pair_counts_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, cut2s, out_perm: torch.Tensor,
                    period: tuple[float, float, float] | None = None,
                    stats: torch.Tensor | None = None) -> torch.Tensor:
    """The pair counts (radius_profile.hip, sum mode) on the current stream: int64 [B] on the
    tree's device, the column sums of radius_profile_gpu, without its [nq, B] array: every block
    writes one row of bin sums into a workspace of nq / 256 rows, which one small kernel adds.
    Arguments as for radius_profile_gpu."""
    return _profile_slices("pair_counts", tree, qsorted, nq, cut2s, out_perm, period, stats, sums=True)


# --------------------------------------------------------------------------- anisotropic pair counts
PAIRS2D_MODES = {"rppi": 0, "smu": 1}
PAIRS2D_MAX_EDGES = 2048   # pair_counts_2d.hip kMaxEdges: cutoffs per axis
PAIRS2D_MAX_CELLS = 65536  # pair_counts_2d.hip kMaxGrid: cells of the whole grid


def _pairs2d_args(what: str, a2, b2, mode: str, los: int) -> tuple:
    if mode not in PAIRS2D_MODES:
        raise ValueError(f"{what}: mode must be 'rppi' or 'smu' (got {mode!r})")
    if isinstance(los, bool) or los not in (0, 1, 2):
        raise ValueError(f"{what}: los must be 0, 1 or 2 (got {los!r})")
    a, b = _profile_cut2s(what, a2), _profile_cut2s(what, b2)
    if a.shape[0] > PAIRS2D_MAX_EDGES or b.shape[0] > PAIRS2D_MAX_EDGES or \
            a.shape[0] * b.shape[0] > PAIRS2D_MAX_CELLS:
        raise ValueError(f"{what}: at most {PAIRS2D_MAX_EDGES} cutoffs per axis and {PAIRS2D_MAX_CELLS} cells "
                         f"(got {a.shape[0]} x {b.shape[0]})")
    return a, b


def check_observer(what: str, observer) -> tuple[float, float, float]:
    """(ox, oy, oz) as float32 values, each finite. Anything else raises ValueError."""
    if isinstance(observer, torch.Tensor):
        observer = observer.detach().cpu().tolist()
    try:
        vals = tuple(float(torch.tensor(float(v), dtype=torch.float32)) for v in observer)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{what}: observer must be three finite numbers (got {observer!r})") from None
    if len(vals) != 3 or not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{what}: observer must be three finite numbers (got {observer!r})")
    return vals


def _pairs2d_cpu(what: str, points: torch.Tensor, queries: torch.Tensor, a2, b2, mode: str, los, period=None,
                 weights: tuple | None = None, observer: bool = False) -> torch.Tensor:
    """The body of the four oracles below: the checks under the caller's name, then one call of
    lsk_cpu_pair_sums_2d. observer: `los` holds the observer, not an axis (open box: no period);
    weights: None = the counts, else (weights, query_weights or None)."""
    a, b = _pairs2d_args(what, a2, b2, mode, 0 if observer else los)
    obs = check_observer(what, los) if observer else None
    per = None if period is None else check_period(what, period)
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    w = wq = None
    if weights is not None:
        w = int64_weights(what, "weights", weights[0], pts.shape[0]).cpu()
        if weights[1] is not None:
            wq = int64_weights(what, "query_weights", weights[1], q.shape[0]).cpu()
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.int64)
    _native.host().lsk_cpu_pair_sums_2d(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], _ptr(a), a.shape[0], _ptr(b),
                                        b.shape[0], PAIRS2D_MODES[mode], 0 if observer else int(los),
                                        None if per is None else _period_c(per),
                                        None if obs is None else _period_c(obs), _ptr(w), _ptr(wq), _ptr(out),
                                        _nthreads())
    return out


def pair_sums_2d_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, a2, b2, mode: str, los, out_perm: torch.Tensor,
                     period: tuple[float, float, float] | None = None, weights: tuple | None = None,
                     query_weights: torch.Tensor | None = None, stats: torch.Tensor | None = None) -> torch.Tensor:
    """The anisotropic pair counts and weighted pair sums (pair_counts_2d.hip) on the current stream:
    int64 [Ba, Bb] on the tree's device, what the four oracles below define, from one walk per slice
    of 2048 cells; the blocks add their cells to the result, one small kernel makes it cumulative.
    tree / qsorted / out_perm / period / stats as for pair_counts_gpu.
    los: an axis (0, 1, 2), or the observer (three finite numbers): the observer walk, open box; its
    cull is a ball per slice whose radius the library takes from the host copies of the cutoffs, and
    there is no whole-box acceptance (word 3 of stats stays 0).
    weights: None = the counts, else (wsorted, wprefix), int64 [n] / [n + 1], the weights in the
    tree's curve order and their exclusive prefix sum; query_weights: int64 [nq] in query order or
    None, with weights only. The caller guarantees max|w| * n < 2^62 and (sum |w|) * (sum
    |query_weights|) < 2^63. The library refuses query weights without weights and an observer with
    a period (NativeError) before it queues anything."""
    what = "pair_sums_2d_gpu"
    axis = isinstance(los, int)
    a, b = _pairs2d_args(what, a2, b2, mode, los if axis else 0)
    obs = None if axis else check_observer(what, los)
    tv = _walk_view(what, tree, qsorted, nq, out_perm)
    dev = tree[0].device
    _profile_stats(what, stats, period, dev)
    if weights is not None:
        _weighted_args(what, tree, *weights)
    wq = _query_weights_arg(what, query_weights, nq, dev)
    res = torch.empty((a.shape[0], b.shape[0]), dtype=torch.int64, device=dev)
    adev, bdev = a.to(dev), b.to(dev)
    check(_native.hip().lsk_hip_pair_sums_2d(
        C.byref(tv), _ptr(qsorted), int(nq), _ptr(adev), None if axis else _ptr(a), a.shape[0], _ptr(bdev),
        None if axis else _ptr(b), b.shape[0], PAIRS2D_MODES[mode], int(los) if axis else 0,
        None if period is None else _period_c(period), None if axis else _period_c(obs), _ptr(out_perm),
        *(_ptr(t) for t in weights or (None, None)), _ptr(wq), _ptr(res), _ptr(stats), _stream(tree[0])),
        "pair_sums_2d")
    return res


def pair_counts_2d_cpu(points: torch.Tensor, queries: torch.Tensor, a2, b2, mode: str, los: int = 2,
                       period=None) -> torch.Tensor:
    """CPU oracle (brute force over all pairs) of the anisotropic pair counts: int64 [Ba, Bb],
    cumulative on both axes. mode 'rppi': S[i, j] = #{pairs : perp2 < a2[i] and par2 < b2[j]};
    'smu': #{pairs : d2 < a2[i] and par2 < b2[j] * d2}, with par2 = dl * dl of the line-of-sight
    axis `los` of the float32 differences q - p (period: their minimum image), perp2 = fmaf(db,
    db, da * da) of the other two. a2 / b2: ascending squared cutoffs (sequences or CPU tensors)."""
    return _pairs2d_cpu("pair_counts_2d_cpu", points, queries, a2, b2, mode, los, period)


def pair_counts_2d_observer_cpu(points: torch.Tensor, queries: torch.Tensor, a2, b2, mode: str,
                                observer=(0.0, 0.0, 0.0)) -> torch.Tensor:
    """CPU oracle (brute force over all pairs) of the anisotropic pair counts with the line of sight
    of an observer: pair_counts_2d_cpu in the open box with, per pair, l = (q - o) + (p - o) per
    axis (twice the vector observer -> midpoint), sl = fmaf(dz, lz, fmaf(dy, ly, dx * lx)), ll =
    dist2(l), par2 = (sl / ll) * sl and perp2 = d2 - par2 (a negative one becomes 0, a NaN stays),
    all float32. A pair whose midpoint is the observer counts nowhere."""
    return _pairs2d_cpu("pair_counts_2d_observer_cpu", points, queries, a2, b2, mode, observer, observer=True)


# --------------------------------------------------------------------------- weighted radius profiles
def int64_weights(what: str, name: str, w, count: int, device: torch.device | None = None) -> torch.Tensor:
    """The int64 [count] weight tensor `name` of the function `what`, checked and contiguous (also
    knn_engine's check); device: where it must live (None: anywhere). ValueError otherwise."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.int64 or w.dim() != 1 or w.shape[0] != count:
        got = f"{w.dtype} {tuple(w.shape)}" if isinstance(w, torch.Tensor) else type(w).__name__
        raise ValueError(f"{what}: {name} must be an int64 [{count}] tensor (got {got})")
    if device is not None and w.device != device:
        raise ValueError(f"{what}: {name} on {w.device}, the index on {device}")
    return w.contiguous()


def weighted_profile_cpu(points: torch.Tensor, queries: torch.Tensor, cut2s, weights: torch.Tensor,
                         period=None) -> torch.Tensor:
    """CPU oracle (brute force over all pairs): int64 [nq, B], column b = the sum of weights[i]
    over the rows i of `points` with dist2 < cut2s[b] (strict; with `period` the minimum-image
    distance), summed per shell and then prefix-summed. weights: int64 [n], one per row of
    `points`, negative allowed; the sums wrap in 64 bits (exact when sum |w| < 2^63). With unit
    weights this is radius_profile_cpu."""
    c = _profile_cut2s("weighted_profile_cpu", cut2s)
    per = None if period is None else check_period("weighted_profile_cpu", period)
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    w = int64_weights("weighted_profile_cpu", "weights", weights, pts.shape[0]).cpu()
    out = torch.empty((q.shape[0], c.shape[0]), dtype=torch.int64)
    _native.host().lsk_cpu_weighted_profile(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], _ptr(c), c.shape[0],
                                            None if per is None else _period_c(per), _ptr(w), _ptr(out),
                                            _nthreads())
    return out


def weighted_pair_sums_cpu(points: torch.Tensor, queries: torch.Tensor, cut2s, weights: torch.Tensor,
                           period=None, query_weights: torch.Tensor | None = None) -> torch.Tensor:
    """CPU oracle of the weighted pair sums: int64 [B], the sum over the queries of
    query_weights[q] (int64 [nq]; None: 1) times row q of weighted_profile_cpu."""
    prof = weighted_profile_cpu(points, queries, cut2s, weights, period)
    if query_weights is not None:
        wq = int64_weights("weighted_pair_sums_cpu", "query_weights", query_weights, prof.shape[0]).cpu()
        prof = prof * wq[:, None]
    return prof.sum(0, dtype=torch.int64)


def weighted_profile_bins() -> int:
    """Cutoffs per launch of radius_profile.hip's weight policy; longer lists go in slices."""
    return int(_native.hip().lsk_hip_weighted_profile_bins())


def _weighted_args(what: str, tree: tuple, wsorted: torch.Tensor, wpre: torch.Tensor) -> None:
    n, dev = tree[3], tree[0].device
    for name, t, count in (("wsorted", wsorted, n), ("wpre", wpre, n + 1)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.shape[0] != count or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{what}: {name} must be a contiguous int64 [{count}] tensor on the tree's device")


def weighted_profile_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, cut2s, out_perm: torch.Tensor,
                         wsorted: torch.Tensor, wpre: torch.Tensor,
                         period: tuple[float, float, float] | None = None,
                         stats: torch.Tensor | None = None) -> torch.Tensor:
    """The weighted radius profile (radius_profile.hip, the weight policy) on the current stream:
    int64 [nq, B] in query order, column b = the sum of the weights of the points with dist2 <
    cut2s[b], from one walk per slice of up to weighted_profile_bins() cutoffs. wsorted: int64 [n],
    the weights in the tree's curve order; wpre: int64 [n + 1], their exclusive prefix sum. The
    caller guarantees max|w| * n < 2^62. Everything else as for radius_profile_gpu."""
    return _profile_slices("weighted_profile", tree, qsorted, nq, cut2s, out_perm, period, stats, sums=False,
                           weights=(wsorted, wpre))


def weighted_pair_sums_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, cut2s, out_perm: torch.Tensor,
                           wsorted: torch.Tensor, wpre: torch.Tensor, query_weights: torch.Tensor | None = None,
                           period: tuple[float, float, float] | None = None,
                           stats: torch.Tensor | None = None) -> torch.Tensor:
    """The weighted pair sums (radius_profile.hip, the weight policy in sum mode) on the current
    stream: int64 [B] on the tree's device, the sum over the queries of query_weights[q] (int64
    [nq] in query order; None: 1) times row q of weighted_profile_gpu, without its [nq, B] array.
    The caller guarantees (sum |w|) * (sum |query_weights|) < 2^63. Arguments as for
    weighted_profile_gpu."""
    return _profile_slices("weighted_pair_sums", tree, qsorted, nq, cut2s, out_perm, period, stats, sums=True,
                           weights=(wsorted, wpre), query_weights=query_weights)


def weighted_pair_sums_2d_cpu(points: torch.Tensor, queries: torch.Tensor, a2, b2, weights: torch.Tensor, mode: str,
                              los: int = 2, period=None, query_weights: torch.Tensor | None = None) -> torch.Tensor:
    """CPU oracle (brute force over all pairs) of the weighted anisotropic pair sums: int64 [Ba, Bb],
    cumulative on both axes, pair_counts_2d_cpu with query_weights[q] * weights[p] added per pair in
    the place of 1. weights: int64 [n], one per row of `points`; query_weights: int64 [nq] or None
    (all ones); negative allowed. Sums and products wrap in 64 bits (exact when (sum |w|) * (sum
    |wq|) < 2^63). With unit weights this is pair_counts_2d_cpu."""
    return _pairs2d_cpu("weighted_pair_sums_2d_cpu", points, queries, a2, b2, mode, los, period,
                        (weights, query_weights))


def weighted_pair_sums_2d_observer_cpu(points: torch.Tensor, queries: torch.Tensor, a2, b2, weights: torch.Tensor,
                                       mode: str, observer=(0.0, 0.0, 0.0),
                                       query_weights: torch.Tensor | None = None) -> torch.Tensor:
    """CPU oracle of the weighted anisotropic pair sums with the line of sight of an observer:
    pair_counts_2d_observer_cpu with query_weights[q] * weights[p] added per pair in the place of 1,
    weights and wrapping as for weighted_pair_sums_2d_cpu."""
    return _pairs2d_cpu("weighted_pair_sums_2d_observer_cpu", points, queries, a2, b2, mode, observer,
                        weights=(weights, query_weights), observer=True)


# --------------------------------------------------------------------------- periodic k-NN
def kth_periodic_cpu(points: torch.Tensor, queries: torch.Tensor, k: int, cut2: float, period) -> torch.Tensor:
    """CPU oracle (brute force): kth_cpu with the periodic squared distance of
    radius_periodic_count_cpu: float32 [nq], per query the k-th smallest pd2 among those < cut2,
    cut2 when fewer than k qualify."""
    if k < 1:
        raise ValueError("kth_periodic_cpu: k must be at least 1")
    per = check_period("kth_periodic_cpu", period)
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    out = torch.empty(q.shape[0], dtype=torch.float32)
    _native.host().lsk_cpu_kth_periodic(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], int(k), C.c_float(cut2),
                                        _period_c(per), _ptr(out), _nthreads())
    return out


def knn_periodic_cpu(points: torch.Tensor, queries: torch.Tensor, k: int, cut2: float,
                     period) -> tuple[torch.Tensor, torch.Tensor]:
    """CPU oracle of the periodic neighbour lists (brute force): knn_cpu with the periodic squared
    distance, the same order, tie rule and unfilled slots. d2[:, k - 1] equals kth_periodic_cpu."""
    if k < 1:
        raise ValueError("knn_periodic_cpu: k must be at least 1")
    per = check_period("knn_periodic_cpu", period)
    pts = points.contiguous().float().cpu()
    q = queries.contiguous().float().cpu()
    idx = torch.empty((q.shape[0], k), dtype=torch.int32)
    d2 = torch.empty((q.shape[0], k), dtype=torch.float32)
    _native.host().lsk_cpu_knn_periodic(_ptr(pts), pts.shape[0], _ptr(q), q.shape[0], int(k), C.c_float(cut2),
                                        _period_c(per), _ptr(idx), _ptr(d2), _nthreads())
    return idx, d2


def mst_periodic_cpu(points: torch.Tensor, period, core_d2: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """CPU oracle of the periodic minimum spanning tree: mst_cpu with dist2 replaced by the
    periodic squared distance of radius_periodic_count_cpu (symmetric in its bits), whatever the
    length of an edge and wherever the coordinates lie."""
    per = check_period("mst_periodic_cpu", period)
    pts = points.contiguous().float().cpu()
    n = pts.shape[0]
    core = None
    if core_d2 is not None:
        core = core_d2.contiguous().float().cpu()
        if core.dim() != 1 or core.shape[0] != n or not bool((torch.isfinite(core) & (core >= 0)).all()):
            raise ValueError("mst_periodic_cpu: core_d2 must hold n finite entries >= 0")
    rows = torch.empty((max(n - 1, 0), 2), dtype=torch.int32)
    d2 = torch.empty(max(n - 1, 0), dtype=torch.float32)
    m = int(_native.host().lsk_cpu_mst_periodic(_ptr(pts), n, _ptr(core), _period_c(per), _ptr(rows), _ptr(d2)))
    return rows[:m].contiguous(), d2[:m].contiguous()


def _pknn_view(what: str, tree: tuple, qsorted: torch.Tensor, nq: int, **arrays) -> TreeView:
    """The view of `tree` for the periodic k-NN passes; arrays: name = (tensor, dtype, least size)."""
    pts, nodes, qnodes, n, depth = tree
    if qsorted.shape[0] < nq or qsorted.device != pts.device:
        raise ValueError(f"{what}: qsorted [>= nq, 3] on the tree's device")
    for name, (t, dt, cnt) in arrays.items():
        if t.dtype != dt or t.numel() < cnt or not t.is_contiguous() or t.device != pts.device:
            raise ValueError(f"{what}: {name} must be {dt} [>= {cnt}], contiguous, on the tree's device")
    return TreeView(_ptr(pts), _ptr(nodes), _ptr(qnodes), n, depth, 0)


def pknn_flag_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, d2: torch.Tensor, cut2: float,
                  period: tuple[float, float, float]) -> tuple[torch.Tensor, torch.Tensor]:
    """The flag pass of the periodic k-NN (knn_periodic.hip): (cutq float32 [nq], flags int32 [nq]),
    both in the order of the curve-sorted queries, from their open-box k-th squared distances d2.
    cutq: the closed bound d2 as a strict cutoff; flags: 1 where a wrapped point may lie below it."""
    tv = _pknn_view("pknn_flag_gpu", tree, qsorted, nq, d2=(d2, torch.float32, nq))
    dev = tree[0].device
    cutq = torch.empty(nq, dtype=torch.float32, device=dev)
    flags = torch.empty(nq, dtype=torch.int32, device=dev)
    check(_native.hip().lsk_hip_pknn_flag(C.byref(tv), _ptr(qsorted), _ptr(d2), int(nq), C.c_float(cut2),
                                          _period_c(period), _ptr(cutq), _ptr(flags), _stream(tree[0])), "pknn_flag")
    return cutq, flags


def pknn_count_gpu(tree: tuple, qsorted: torch.Tensor, nq: int, qlist: torch.Tensor, cutq: torch.Tensor,
                   period: tuple[float, float, float], stats: torch.Tensor | None = None) -> torch.Tensor:
    """The count pass over the flagged list: int32 [m], per entry of qlist (int32, ascending
    positions of the curve-sorted queries) the number of points with pd2 < cutq[entry]. stats:
    optional zeroed int64 [RADIUS_PERIODIC_STATS]."""
    m = qlist.numel()
    tv = _pknn_view("pknn_count_gpu", tree, qsorted, nq, qlist=(qlist, torch.int32, m), cutq=(cutq, torch.float32, nq))
    counts = torch.empty(m, dtype=torch.int32, device=tree[0].device)
    check(_native.hip().lsk_hip_pknn_count(C.byref(tv), _ptr(qsorted), _ptr(qlist), int(m), _ptr(cutq),
                                           _period_c(period), _ptr(counts), _ptr(stats), _stream(tree[0])),
          "pknn_count")
    return counts


def pknn_fill_gpu(tree: tuple, perm: torch.Tensor, qsorted: torch.Tensor, nq: int, qlist: torch.Tensor,
                  cutq: torch.Tensor, period: tuple[float, float, float], offsets: torch.Tensor, total: int,
                  err: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The fill pass of pknn_rows_gpu, also on its own: (idx int32 [total], pd2 float32 [total]),
    the rows `offsets` in walk order with the periodic squared distances as the walk computed
    them (no sort, no square root)."""
    m = qlist.numel()
    tv = _pknn_view("pknn_fill_gpu", tree, qsorted, nq, qlist=(qlist, torch.int32, m), cutq=(cutq, torch.float32, nq),
                    perm=(perm, torch.int32, tree[3]), offsets=(offsets, torch.int64, m + 1),
                    err=(err, torch.int32, 1))
    if offsets.numel() != m + 1:
        raise ValueError("pknn_fill_gpu: offsets must be [m + 1]")
    dev = tree[0].device
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    pd2 = torch.empty(total, dtype=torch.float32, device=dev)
    check(_native.hip().lsk_hip_pknn_fill(C.byref(tv), _ptr(perm), _ptr(qsorted), _ptr(qlist), int(m), _ptr(cutq),
                                          _period_c(period), _ptr(offsets), _ptr(idx), _ptr(pd2), _ptr(err),
                                          _stream(tree[0])), "pknn_fill")
    return idx, pd2


def pknn_rows_gpu(tree: tuple, perm: torch.Tensor, qsorted: torch.Tensor, nq: int, qlist: torch.Tensor,
                  cutq: torch.Tensor, period: tuple[float, float, float], offsets: torch.Tensor, total: int,
                  longest: int, qperm: torch.Tensor, d2: torch.Tensor, cut2: float, k: int, out: torch.Tensor,
                  out_idx: torch.Tensor | None, out_dist: torch.Tensor | None, err: torch.Tensor) -> None:
    """Fill, sort and take for one slice of the flagged list: the rows `offsets` (int64 [m + 1],
    from pknn_count_gpu's counts of this slice; total = offsets[m], longest >= the longest row)
    are filled, sorted by lsk_hip_radius_sort, and their first k overwrite out[qperm[q]] (and
    rows qperm[q] of out_idx / out_dist [nq, k], when given) of the slice's queries. err: the
    device error word (int32 [1], accumulated over the slices)."""
    m = qlist.numel()
    arrays = dict(qlist=(qlist, torch.int32, m), cutq=(cutq, torch.float32, nq), perm=(perm, torch.int32, tree[3]),
                  offsets=(offsets, torch.int64, m + 1), qperm=(qperm, torch.int32, nq), d2=(d2, torch.float32, nq),
                  out=(out, torch.float32, nq), err=(err, torch.int32, 1))
    if out_idx is not None:
        arrays.update(out_idx=(out_idx, torch.int32, nq * k), out_dist=(out_dist, torch.float32, nq * k))
    tv = _pknn_view("pknn_rows_gpu", tree, qsorted, nq, **arrays)
    if offsets.numel() != m + 1 or k < 1:
        raise ValueError("pknn_rows_gpu: offsets must be [m + 1] and k >= 1")
    lib, st = _native.hip(), _stream(tree[0])
    idx, dist = pknn_fill_gpu(tree, perm, qsorted, nq, qlist, cutq, period, offsets, total, err)
    check(lib.lsk_hip_radius_sort(_ptr(offsets), int(m), int(total), int(longest), _ptr(idx), _ptr(dist), 1, st),
          "radius_sort")
    check(lib.lsk_hip_pknn_take(_ptr(qlist), int(m), _ptr(offsets), _ptr(idx), _ptr(dist), _ptr(qperm), _ptr(d2),
                                C.c_float(cut2), int(k), _ptr(out), _ptr(out_idx), _ptr(out_dist), _ptr(err), st),
          "pknn_take")


# --------------------------------------------------------------------------- halo
UB_MAX_W = 8  # tree.hip kUbMaxW: beyond it the box-pair bound


def tree_set_radii_ub(nodes: torch.Tensor, pts: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """Per-node upper bound of the k-th squared radius before any query ran (tree.hip
    leaf_radius_ub_kernel): the ceil(k/64)+1 buckets around a leaf hold >= k points;
    with m(p) = farthest-corner distance from window point p to the leaf box, the k-th
    smallest m(p) bounds every leaf query's k-th neighbour distance (beyond UB_MAX_W
    buckets: the farthest corner pair of the leaf box and the window's union box).
    `pts`: the index's sorted points."""
    if is_gpu(nodes):
        check(_native.hip().lsk_hip_tree_set_radii_ub(_ptr(nodes), _ptr(pts), n, k, _stream(nodes)),
              "tree_set_radii_ub")
        return nodes
    depth = tree_depth(n)
    slots = 1 << depth
    nb = (n + BUCKET - 1) // BUCKET
    r = torch.zeros(slots, dtype=torch.float32)
    if nb and n < k:
        r[:nb] = math.inf
    elif nb:
        w = min(nb, (k + BUCKET - 1) // BUCKET + 1)
        leaf = torch.arange(nb)
        st = (leaf - (w - 1) // 2).clamp(0, nb - w)
        lo = nodes[slots:slots + nb, 0:3]
        hi = nodes[slots:slots + nb, 4:7]
        if w <= UB_MAX_W:
            idx = (st[:, None] * BUCKET + torch.arange(w * BUCKET)[None, :])   # [nb, 64w]
            valid = idx < n
            p = pts[:n][idx.clamp(max=n - 1)]                                   # [nb, 64w, 3]
            e = torch.maximum(p - lo[:, None, :], hi[:, None, :] - p)
            m = torch.addcmul(torch.addcmul(e[..., 0] * e[..., 0], e[..., 1], e[..., 1]), e[..., 2], e[..., 2])
            m = torch.where(valid, m, torch.full_like(m, math.inf))
            d2 = m.kthvalue(k, dim=1).values
        else:
            win = st[:, None] + torch.arange(w)[None, :]
            wlo = lo[win].amin(dim=1)
            whi = hi[win].amax(dim=1)
            e = torch.maximum(whi - lo, hi - wlo)
            d2 = torch.addcmul(torch.addcmul(e[:, 0] * e[:, 0], e[:, 1], e[:, 1]), e[:, 2], e[:, 2])
        r[:nb] = d2 * (1.0 + 2.0 ** -16)
    nodes[slots:, 3] = r
    return _levelup_radii(nodes, depth)


def boundary_groups(local_nodes: torch.Tensor, depth: int, ngroups: int, pub: torch.Tensor, pub_off: list[int],
                    pub_depth, self_rank: int) -> torch.Tensor:
    """int32 [ngroups]: 1 for the local query groups (buckets) whose leaf box, inflated by
    its squared radius bound (lo.w of local_nodes), comes closer than that bound to some
    node of another rank's published tree (halo.hip boundary_groups_kernel); 0 = the
    group's k nearest are all local, whatever the other ranks hold."""
    nranks = len(pub_off)
    flags = torch.zeros(max(ngroups, 0), dtype=torch.int32, device=local_nodes.device)
    if ngroups <= 0:
        return flags
    if is_gpu(local_nodes):
        off = torch.tensor(pub_off, dtype=torch.int64, device=local_nodes.device)
        dep = (pub_depth.to(device=local_nodes.device, dtype=torch.int32).contiguous()
               if isinstance(pub_depth, torch.Tensor)
               else torch.tensor(pub_depth, dtype=torch.int32, device=local_nodes.device))
        check(_native.hip().lsk_hip_boundary_groups(_ptr(local_nodes), int(depth), int(ngroups), _ptr(pub),
                                                    _ptr(off), _ptr(dep), nranks, self_rank, _ptr(flags),
                                                    _stream(local_nodes)), "boundary_groups")
        return flags
    # CPU: every group against the leaf level of each published tree, in float64 with the
    # squared gap shrunk by 2^-20 (a rounding of the canonical float d² cannot hide a
    # neighbour: the test only errs towards "boundary")
    if isinstance(pub_depth, torch.Tensor):
        pub_depth = [int(x) for x in pub_depth.cpu().tolist()]
    pub = pub.reshape(-1, 8)
    leaves = local_nodes[(1 << depth):(1 << depth) + ngroups].double()
    lo, hi, r2 = leaves[:, None, 0:3], leaves[:, None, 4:7], leaves[:, 3]
    hit = torch.zeros(ngroups, dtype=torch.bool)
    for j in range(nranks):
        if j == self_rank:
            continue
        d = pub_depth[j]
        base = pub_off[j] // 8
        nb = pub[base + (1 << d): base + (2 << d)].double()
        for s0 in range(0, ngroups, 4096):
            gap = torch.clamp(torch.maximum(lo[s0:s0 + 4096] - nb[None, :, 4:7], nb[None, :, 0:3] - hi[s0:s0 + 4096]),
                              min=0.0)
            g2 = (gap * gap).sum(-1) * (1.0 - 2.0 ** -20)
            hit[s0:s0 + 4096] |= (g2 < r2[s0:s0 + 4096, None]).any(1)
    flags[hit] = 1
    return flags


def compact_flags(flags: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(list of the indices i with flags[i] != 0, their count as an int32 [1] tensor on the
    flags' device: no host read on the GPU)."""
    n = flags.shape[0]
    if is_gpu(flags):
        lst = torch.empty(max(n, 1), dtype=torch.int32, device=flags.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=flags.device)
        if n:
            check(_native.hip().lsk_hip_compact_flags(_ptr(flags), n, _ptr(lst), _ptr(cnt), _stream(flags)),
                  "compact_flags")
        return lst, cnt
    idx = torch.nonzero(flags != 0).view(-1).to(torch.int32)
    return idx, torch.tensor([idx.shape[0]], dtype=torch.int32)


def halo_mask(pts: torch.Tensor, pub: torch.Tensor, pub_off: list[int], pub_depth, self_rank: int) -> torch.Tensor:
    """Per point bitmask of ranks whose published radius-inflated boxes contain it.
    pub_depth: published tree depth per rank (list, or an int32 tensor — a device tensor
    keeps the GPU path free of a host read)."""
    n = pts.shape[0]
    nranks = len(pub_off)
    mask = torch.empty(n, dtype=torch.int64, device=pts.device)
    if isinstance(pub_depth, torch.Tensor) and not (is_gpu(pts) and pub_depth.device == pts.device):
        pub_depth = [int(x) for x in pub_depth.cpu().tolist()]
    if is_gpu(pts):
        off = torch.tensor(pub_off, dtype=torch.int64, device=pts.device)
        dep = (pub_depth.to(torch.int32).contiguous() if isinstance(pub_depth, torch.Tensor)
               else torch.tensor(pub_depth, dtype=torch.int32, device=pts.device))
        check(_native.hip().lsk_hip_halo_mask(_ptr(pts), n, _ptr(pub), _ptr(off), _ptr(dep), nranks,
                                              self_rank, _ptr(mask), _stream(pts)), "halo_mask")
        return mask
    # CPU: test against the leaf level of each published tree
    if nranks > 64:  # one mask bit per rank, as lsk_hip_halo_mask (the host loop stops at 64)
        raise ValueError("halo_mask: at most 64 ranks")
    boxes, offs = [], [0]
    pub = pub.reshape(-1, 8)
    for j in range(nranks):
        d = pub_depth[j]
        base = pub_off[j] // 8
        leaves = pub[base + (1 << d): base + (2 << d)]
        boxes.append(leaves)
        offs.append(offs[-1] + leaves.shape[0])
    allb = torch.cat(boxes).contiguous() if boxes else torch.zeros((0, 8))
    offs_t = torch.tensor(offs, dtype=torch.int64)
    _native.host().lsk_cpu_halo_mask(_ptr(pts.contiguous()), n, _ptr(allb), _ptr(offs_t), nranks, self_rank,
                                     _ptr(mask), _nthreads())
    return mask
