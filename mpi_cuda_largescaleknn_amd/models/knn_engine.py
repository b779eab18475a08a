"""Single-rank k-th-nearest-neighbour distance engine.

The "model" of this framework is the reference's per-rank work (SURVEY §1, L2+L4):
build a k-d tree over the rank's points (cukd::buildTree, unorderedDataVariant.cu:161)
and answer one k-NN query per point (runQuery/extractFinalResult, :75-103). Pipeline
on the GPU — every step a hand-written gfx950 kernel on torch's current stream:

    bounds -> Hilbert keys -> LSD radix sort -> gather -> bucket tree (+ cell grid) -> radix-select k-NN

``LocalIndex`` is the reusable product of the first five steps (also used for the
halo tree in the distributed pipelines).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np
import torch

from .._native import NativeError
from ..ops import kernels as K


def cut2_of(max_radius: float) -> float:
    """The reference stores maxRadius as float and compares squared distances against
    cutOff*cutOff evaluated in float (FlexHeapCandidateList init, U:84-85)."""
    r = np.float32(max_radius)
    with np.errstate(over="ignore"):
        return float(r * r)


SEED_BUCKETS = 1  # curve-neighbour buckets (each side) that seed the first pass (1e8 k=100: 0/1/2 -> 0.126/0.125/0.126 s)
KNN_IMPL = "rows"  # "rows" (production kernel + exact backstop) or "exact" (backstop only)
DEBUG_FAIL_MOD = 0  # tests: make the rows kernel hand every m-th query to the backstop
# HIP-graph captures: the failure words of captured launches, checked after a replay
# (verify_captured_failures) — during a capture the host cannot read them. A replay
# re-zeroes each launch's counter, so every captured launch also folds its count into a
# peak slot of CAPTURE_PEAKS (allocated and zeroed by prepare_capture, outside the graph):
# the check then covers every replay, not only the last one.
CAPTURED_FAIL_WORDS: list = []
CAPTURE_PEAKS: torch.Tensor | None = None


def prepare_capture(device: torch.device, slots: int = 64) -> None:
    """Call before capturing k-NN launches into a graph (see CAPTURED_FAIL_WORDS)."""
    global CAPTURE_PEAKS
    CAPTURE_PEAKS = torch.zeros(slots, dtype=torch.int64, device=device)


@dataclass
class KnnConfig:
    k: int
    max_radius: float = math.inf
    publish_levels: int = 15       # top tree levels published for halo filtering (~1K pts/box)
    collect_stats: bool = False

    @property
    def cut2(self) -> float:
        return cut2_of(self.max_radius)


# Cell-grid candidate source of the local k-NN pass (knn_grid.hip): "auto" = built for
# GPU indexes whose sub-cell populations look near-uniform (GRID_CROWD), "on" = always,
# "off" = never (the bucket-tree kernel knn_rows serves every query).
GRID = os.environ.get("LSKNN_GRID", "auto")
GRID_MS = float(os.environ.get("LSKNN_GRID_MS", "6"))  # target mean points per finest cell
# auto: a point's sub-cell holds on average at most this many times the mean (+1)
GRID_CROWD = float(os.environ.get("LSKNN_GRID_CROWD", "2"))
# Which kernel the device gate is expected to pick (the last decision read on the host):
# that one gets the full launch, the other a small persistent one (kernels.knn_gpu).
GRID_EXPECT = [True]


@dataclass
class GridIndex:
    slots: torch.Tensor      # int32 [8^level * 64, 4]: per level-`level` cell, its 64
                             # grandchildren's runs of the sorted array in curve order
    level: int               # cell level (grandchildren at level + 2)
    box: torch.Tensor        # the cube of the sort keys (device)
    inf4: torch.Tensor | None = None  # 4 x +inf on the device (candidate padding)
    gate: torch.Tensor | None = None  # device int32 [1]: 1 = the grid applies (decided on
                                      # the device, GRID=auto), None = always (GRID=on)
    census: tuple | None = None       # (level counts, crowding sum) the gate came from

    def view(self) -> tuple:
        if self.inf4 is None:
            self.inf4 = torch.full((4,), math.inf, dtype=torch.float32, device=self.slots.device)
        return (self.slots, self.level, self.box, self.inf4, self.gate)

    def decision(self) -> dict:
        """Host read of what the device decided from (debugging / reporting)."""
        out = {"level": self.level + 2, "applies": self.applies()}
        if self.census is not None:
            c = [int(x) for x in self.census[0].cpu().tolist()]
            out.update(distinct_g=c[self.level + 2] + 1, distinct_g1=c[self.level + 1] + 1,
                       crowd_sum=int(self.census[1].item()))
        return out

    def applies(self) -> bool:
        """Host read of the device decision (reporting only; never on the hot path)."""
        return self.gate is None or bool(int(self.gate.item()))


@dataclass
class LocalIndex:
    n: int
    pts: torch.Tensor        # [n + PAD, 3] curve-sorted (Hilbert) points (padded)
    perm: torch.Tensor       # int32 [n]: sorted position -> row of the input array
    nodes: torch.Tensor      # [2^(depth+1), 8] bucket-tree node boxes (lo.w = radius²)
    qnodes: torch.Tensor     # [2^depth * 4, 8] boxes of each bucket's four 16-point quarters
    depth: int
    box: torch.Tensor        # [8] cube used for the curve keys
    grid: GridIndex | None = None
    qrot: torch.Tensor | None = None  # [n + PAD, 3]: the sorted points in the rotated frame the
                                      # keys, tree boxes and box tests use (flat_frame), or None
    bkeys: torch.Tensor | None = None  # int32 [ceil(n / 64)]: curve key of sorted point 64 b
                                       # (bucket_keys: built by the first foreign query)
    line: bool = False       # sorted by line_keys (a LineAxis frame), not by the curve of `box`

    @property
    def device(self) -> torch.device:
        return self.pts.device

    def tree(self) -> tuple:
        return (self.pts, self.nodes, self.qnodes, self.n, self.depth)


@dataclass
class KnnStats:
    counters: dict = field(default_factory=dict)

    def add(self, raw: torch.Tensor) -> None:
        names = ["evals", "leaves", "nodes", "hist_passes", "overflow_lanes", "underflow_lanes",
                 "refine_lanes", "mismatch_lanes", "pass_limit_waves", "list_invalid_waves", "waves",
                 "hint_lanes", "recorded_leaves", "collect_steps", "collect_nodes", "guard_trips",
                 # cycle profile (LSK_PROFILE kernel builds only)
                 "prof_proc_hist", "prof_proc_collect", "prof_walk_hist", "prof_walk_collect",
                 "prof_quarters", "prof_inner_nodes", "prof_select", "prof_wave",
                 "prof_rows_entry", "prof_rows_in", "failed_lanes", "binovf_lanes",
                 "prof_dead_slots", "prof_slots", "prof_crows_entry", "prof_crows_in"]
        vals = raw.cpu().tolist()
        for i, nm in enumerate(names):
            self.counters[nm] = self.counters.get(nm, 0) + int(vals[i])

    def add_fallback(self, n: int) -> None:
        self.counters["fallback_queries"] = self.counters.get("fallback_queries", 0) + int(n)


# The point gather fused into the key sort's last pass (kernels.sort_keys_iota_gather)
# instead of a gather3 pass over the permutation: 1B build 74.9 vs 71.9 ms,
# bench neutral (profiles/r6_sort/), so off by default.
FUSED_GATHER = os.environ.get("LSKNN_FUSED_GATHER", "0") == "1"


# Flat data in any orientation (a tilted plane, a slanted line): the bucket tree's axis-
# aligned boxes around a slanted patch are as thick as they are wide, so they cull like 3-D
# boxes around 2-D data (2e7 points, k = 100: tilted plane 649.6 vs axis-aligned plane
# 1239.0 Mpts/s). flat_frame finds the principal axes of such a set; build_index then sorts
# and boxes the points in that frame (keys, tree boxes, box tests) while every distance stays
# canonical in the points' own coordinates, so outputs are bit-identical. The boxes are
# widened by a bound on the rotation's rounding (rotate_margin): culling stays conservative.
# 0: off (A/B).
FLAT_FRAME = os.environ.get("LSKNN_FLAT_FRAME", "1") != "0"
FLAT_RATIO = 1e-6        # smallest / largest principal variance of a flat set
FRAME_SAMPLE = 1 << 13   # points sampled for the covariance (strided)
# The frame pays from k ~ 48 (2e7 tilted plane, k = 100: 647 -> 1012 Mpts/s; k = 16: 1485 ->
# 1366, the rotated build's extra passes outweigh its cheaper walk); the probe is then read
# before the build (FRAME_EARLY: non-flat data pay a ~1 % host wait; read after the build
# instead, a plane pays a wasted build: 911 vs 1012). profiles/r6_nonuniform/flat_frame_ab.txt
FRAME_MIN_K = int(os.environ.get("LSKNN_FRAME_MIN_K", "48"))
FRAME_EARLY = os.environ.get("LSKNN_FRAME_EARLY", "1") == "1"
# ... and only while the plane's k-NN radius (sqrt(k * area / (pi * n))) is >= FRAME_RADIUS_X
# times the boxes' widening (rotate_margin); measured wins down to a ratio of ~4 (5e8, k = 48).
FRAME_RADIUS_X = float(os.environ.get("LSKNN_FRAME_RADIUS_X", "2"))
# ... and only while the square of that widening is a normal float32. A rotated box culls by
# its float32 squared distance against canonical squared distances; the widening m covers the
# two frames' difference by leaving d2 - gap2 >= (m / 2)^2. Below the normal range a squared
# distance rounds by an absolute 2^-150 per operation instead of a relative 2^-24, and once
# m^2 is down there the rounding outweighs the widening: a box that holds the k-th neighbour
# is culled (coordinates of ~2^-70: 4 of 20 000 k = 100 distances of a tilted plane wrong).
FRAME_MIN_MARGIN2 = 2.0 ** -126
# Curve keys in the plane's frame: above PLANE_2D_MIN points, 2-D Morton keys of the two
# in-plane coordinates, 15 bits each — 3-D keys spend a third of their 30 bits on the flat
# axis: 1024^2 cells, ~200 points each at 2e8, wider than the k-NN radius (tilted plane,
# k = 100, 3-D -> 2-D keys: 2e8 379 -> 878, 5e8 167 -> 856 Mpts/s; at 2e7 the 3-D Hilbert
# keys' locality wins, 987 vs 880; profiles/r6_nonuniform/plane_frame_scale.txt). Above it,
# axis-aligned planes take the frame too for the same keys, and every k does (2e8, frame vs
# own: tilted 875 / 1227 vs 630 / 912 at k = 100 / 16, axis-aligned 884 / 1248 vs 649 / 897).
# LSKNN_PLANE_KEYS: auto | 2d | 3d.
PLANE_KEYS = os.environ.get("LSKNN_PLANE_KEYS", "auto")
PLANE_2D_MIN = 1 << 26


# A line (two principal variances negligible) keeps its own frame (rotated fp32 coordinates
# cannot resolve a dense line: profiles/r6_nonuniform/line_frame_ab.txt) but is sorted by its
# position along the axis (line_keys) instead of 3-D curve keys. LSKNN_LINE_KEYS=0: off.
LINE_KEYS = os.environ.get("LSKNN_LINE_KEYS", "1") != "0"


class LineAxis(NamedTuple):
    """FrameProbe's verdict for a line: its unit direction (float32 [3], device)."""
    a: torch.Tensor


def line_keys(points: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """30-bit keys of points by their projection on the direction a (float32 arithmetic:
    ~24 significant bits; ties in any order)."""
    t = points[:, 0] * a[0] + points[:, 1] * a[1] + points[:, 2] * a[2]
    lo, hi = t.min(), t.max()
    t = (t - lo) * (float(1 << 30) / (hi - lo).clamp_min(1e-30))
    return t.clamp_(0.0, float((1 << 30) - 64)).to(torch.int32)


def _plane_2d(n: int) -> bool:
    return PLANE_KEYS == "2d" or (PLANE_KEYS == "auto" and n > PLANE_2D_MIN)


class FrameProbe:
    """The flatness test of flat_frame: a strided sample's 3x3 covariance is computed on
    the device (float64 sums); result() reads it (one small host read) and returns the
    rotation, or None."""

    def __init__(self, points: torch.Tensor, k: int = FRAME_MIN_K):
        self.cov = None
        self.k = k
        n = points.shape[0]
        if not FLAT_FRAME or (k < FRAME_MIN_K and not _plane_2d(n) and not LINE_KEYS) or not K.is_gpu(points) or n < 1024 \
                or _SYNC_FREE[0] \
                or torch.cuda.is_current_stream_capturing():
            return
        smp = points[::max(1, n // FRAME_SAMPLE)][:FRAME_SAMPLE].to(torch.float64)
        self.n, self.m = n, smp.shape[0]
        c = smp - smp.mean(0)
        # (read by result() with one small blocking copy: the probe is read before the build
        # anyway, FRAME_EARLY, so a pinned buffer + event saved nothing)
        self.cov = torch.stack([(c[:, i] * c[:, j]).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2),
                                                                         (2, 2))] + [smp.abs().max()])
        self.device = points.device

    def result(self) -> torch.Tensor | None:
        if self.cov is None:
            return None
        a = self.cov.cpu().numpy()
        cov = np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])
        if not np.isfinite(cov).all():
            return None
        w, v = np.linalg.eigh(cov)  # ascending
        if not (w[2] > 0) or w[0] > FLAT_RATIO * w[2]:
            return None
        if w[1] <= FLAT_RATIO * w[2]:  # a line: sorted along its axis, in its own frame
            return LineAxis(torch.tensor(v[:, 2].copy(), dtype=torch.float32, device=self.device)) \
                if LINE_KEYS else None
        # a plane: one principal variance negligible, the other two not
        if w[1] < 1e-3 * w[2] or (self.k < FRAME_MIN_K and not _plane_2d(self.n)):
            return None
        if np.max(np.abs(v[:, 0])) > 1.0 - 1e-6 and not _plane_2d(self.n):
            return None  # already axis-aligned: the tree is thin as is (3-D keys either way)
        # the k-NN radius against rotate_margin (extents of a uniform spread: sqrt(12 var))
        e1, e2 = math.sqrt(12.0 * w[1] / self.m), math.sqrt(12.0 * w[2] / self.m)
        radius = math.sqrt(self.k * e1 * e2 / (math.pi * max(self.n, 1)))
        margin = (a[6] * 1.7320508 + e2) * 2.0 ** -16
        if radius < FRAME_RADIUS_X * margin or margin * margin < FRAME_MIN_MARGIN2:
            return None
        R = v[:, ::-1].T.copy()  # rows: axes by decreasing variance
        return torch.tensor(R, dtype=torch.float32, device=self.device)


def flat_frame(points: torch.Tensor) -> torch.Tensor | None:
    """3x3 float32 rotation (rows: principal axes, largest variance first) when `points`
    (GPU) lie on a plane that is not already aligned with the coordinate axes, else None
    (FrameProbe, read at once; eager paths only: never inside a HIP-graph capture or a
    stream of sets)."""
    return FrameProbe(points).result()


def rotate(points: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    """points @ R^T with explicit fp32 multiply-adds (no reduced-precision GEMM path)."""
    p0, p1, p2 = points[:, 0:1], points[:, 1:2], points[:, 2:3]
    return p0 * R[:, 0] + p1 * R[:, 1] + p2 * R[:, 2]


def rotate_margin(rbox: torch.Tensor) -> torch.Tensor:
    """Per-side widening of every box built from rotated points (device scalar): bounds the
    difference between distances in the rotated frame (float-evaluated, non-orthonormal
    float matrix) and the canonical float distances in the points' own frame — ~9 ulp of the
    largest coordinate for the rotation, a few ulp of the extent for the distances — with a
    wide safety factor (2^-16 of |coordinate| + extent)."""
    mag = torch.maximum(rbox[0:3].abs(), rbox[3:6].abs()).max()
    ext = (rbox[3:6] - rbox[0:3]).max()
    return (mag * 1.7320508 + ext) * (2.0 ** -16)


def build_index(points: torch.Tensor, box: torch.Tensor | None = None,
                keys: tuple | None = None, grid: bool = False, density_n: int | None = None,
                grid_level: int | None = None, grid_gated: bool = True,
                frame: torch.Tensor | None = None) -> LocalIndex:
    """Sort points along the space-filling curve of `box` (default: their own bounds) and
    build the bucket tree. `keys` = (keys, iota) computed already (SetStream's PRE_KEYS:
    the next set's box and curve keys on the side stream beside the current k-NN). `grid`: also index the sorted points by the cell grid of
    the fast local k-NN pass (build_grid, GPU). `density_n`: the number of points that
    fill `box` (a rank's share of a global box: the global count; default: n).
    `grid_level`: force the grid's grandchild level (tests; a halo index takes the local
    grid's); `grid_gated=False`: no census / device gate for the grid (build_grid).
    `frame` (flat_frame, GPU, with no keys or box given): the index is built in that rotated
    frame (no grid) — see FLAT_FRAME.
    No host read on the way unless an over-full key cell needs the eager refinement
    (refine_heavy_cells; under host_sync_free() not even that)."""
    points = points.contiguous()
    n = points.shape[0]
    line = False
    if isinstance(frame, LineAxis):  # a line: its own frame, keys along its axis, no grid
        if keys is None and K.is_gpu(points) and n >= 2:
            keys, grid, line = (line_keys(points, frame.a), None), False, True
        frame = None
    if frame is not None and K.is_gpu(points) and keys is None and box is None and n >= 2:
        return _build_rotated(points, frame)
    if box is None:
        box = K.bounds(points)
    gpu = K.is_gpu(points)
    spts = None  # points in sorted order, gathered by the sort's last pass (FUSED_GATHER)
    if keys is not None and keys[1] is not None:
        skeys, perm = K.sort_pairs(keys[0], keys[1], 30)
    elif gpu or keys is not None:  # (the sort's first pass generates the values: no iota array)
        kk = keys[0] if keys is not None else K.morton(points, box, with_iota=False)[0]
        if FUSED_GATHER and gpu and n >= 2:
            skeys, perm, spts = K.sort_keys_iota_gather(kk, points, 30, pad=K.PAD_POINTS)
        else:
            skeys, perm = K.sort_keys_iota(kk, 30)
    else:
        skeys, perm = K.sort_pairs(*K.morton(points, box), 30)
    # level census (grid) and over-full-cell flag (refinement) in one pass over the keys
    census = K.key_census(skeys[:n], HEAVY_RUN) if gpu and n > 1 else None
    sorted_perm = perm
    perm = refine_heavy_cells(points, skeys, perm, heavy=census[1] if census is not None else None)
    # (a refinement reorders over-full cells: the fused gather's order is then stale)
    pts = spts if spts is not None and perm is sorted_perm else K.gather3(points, perm, pad=K.PAD_POINTS)
    nodes, qnodes, depth = K.build_tree(pts, n)
    index = LocalIndex(n, pts, perm, nodes, qnodes, depth, box, line=line)
    if grid:
        index.grid = build_grid(index, skeys, density_n, grid_level,
                                counts=census[0] if census is not None else None, gated=grid_gated)
    return index


def _spread15(v: torch.Tensor) -> torch.Tensor:
    """The low 15 bits of int32 v moved to the even bit positions."""
    v = (v | (v << 8)) & 0x00FF00FF
    v = (v | (v << 4)) & 0x0F0F0F0F
    v = (v | (v << 2)) & 0x33333333
    return (v | (v << 1)) & 0x55555555


def plane_keys(rp: torch.Tensor, rbox: torch.Tensor) -> torch.Tensor:
    """30-bit 2-D Morton keys of rotated points by their first two coordinates (the plane's
    own axes), 15 bits each over the square of the larger in-plane extent."""
    s = float(1 << 15) / torch.maximum(rbox[3] - rbox[0], rbox[4] - rbox[1]).clamp_min(1e-30)
    x = ((rp[:, 0] - rbox[0]) * s).clamp_(0.0, 32767.0).to(torch.int32)
    y = ((rp[:, 1] - rbox[1]) * s).clamp_(0.0, 32767.0).to(torch.int32)
    return _spread15(x) | (_spread15(y) << 1)


def _build_rotated(points: torch.Tensor, R: torch.Tensor) -> LocalIndex:
    """build_index in the frame R: curve keys, sort and tree boxes from the rotated points
    (boxes widened by rotate_margin), the index's points (the candidates' coordinates) in
    their own frame, qrot the queries in the rotated one. No grid (flat data)."""
    n = points.shape[0]
    rp = rotate(points, R).contiguous()
    rbox = K.bounds(rp)
    keys = plane_keys(rp, rbox) if _plane_2d(n) else K.morton(rp, rbox, with_iota=False)[0]
    skeys, perm = K.sort_keys_iota(keys, 30)
    census = K.key_census(skeys[:n], HEAVY_RUN) if n > 1 else None
    perm = refine_heavy_cells(rp, skeys, perm, heavy=census[1] if census is not None else None)
    pts = K.gather3(points, perm, pad=K.PAD_POINTS)
    qrot = K.gather3(rp, perm, pad=K.PAD_POINTS)
    nodes, qnodes, depth = K.build_tree(qrot, n)
    m = rotate_margin(rbox)
    for t in (nodes, qnodes):
        t[:, 0:3] -= m
        t[:, 4:7] += m
    return LocalIndex(n, pts, perm, nodes, qnodes, depth, rbox, qrot=qrot)


def grid_level_for(density_n: int, n_local: int, ms: float = GRID_MS) -> int:
    """Grandchild level of the grid from point counts alone (no census, no host read):
    the level whose occupied cells would hold closest to `ms` points on average, in log
    scale, for `density_n` uniform points filling the cube (mean population of the
    occupied cells = lam / (1 - e^-lam), lam = density_n / 8^g; 1B -> 9, 1e8 -> 8,
    1e7 -> 7 — what the census picks for uniform data), then capped so that the slot
    table (16 KiB... 1 KiB per level g-2 cell) stays within 48 B per local point + 64 MiB:
    a rank's share of a large global cube does not allocate the whole cube's finest table
    (a capped level is coarser, hence slower, never wrong)."""
    best, err = 2, math.inf
    for g in range(2, 11):
        lam = max(density_n, 1) / float(8 ** g)
        mean = lam / -math.expm1(-lam) if lam > 1e-12 else 1.0
        e = abs(math.log(max(mean, 1e-9) / ms))
        if e < err:
            best, err = g, e
    while best > 2 and 1024 * 8 ** (best - 2) > 48 * max(n_local, 1) + (64 << 20):
        best -= 1
    return best


def grid_level(distinct: list[int], n: int, ms: float = GRID_MS) -> int:
    """Level of the grid's finest cells (the grandchildren whose runs the k-NN pass
    streams; enumerated through their level-2 ancestors): the level whose occupied cells
    hold closest to `ms` points on average, in log scale (uniform points in a cube, ms = 6:
    1B -> 9 (7.5 per cell), 1e8 -> 8 (6.0), 1e7 -> 7 (4.8)), in [2, 10]. Finer levels cull
    more candidates (at 1e8, k=100: level 8 3.6K evaluations per query vs 4.6K at 7), and
    merged runs keep the segments long."""
    best, err = 2, math.inf
    for lvl in range(2, 11):
        if distinct[lvl] <= 0:
            continue
        e = abs(math.log(max(n / distinct[lvl], 1e-9) / ms))
        if e < err:
            best, err = lvl, e
    return best


def grid_applies(distinct: list[int], n: int, g: int) -> bool:
    """GRID=auto: near-uniform 3-D data at the grid's scale — occupied cells multiply by
    >= 6 from level g-1 to g (planar data: 4, exact copies: 1), and the level's mean
    population is within [2, 256] points."""
    mean = n / max(1, distinct[g])
    return distinct[g] >= 6 * distinct[g - 1] and 2.0 <= mean <= 256.0


def build_grid(index: LocalIndex, skeys: torch.Tensor, density_n: int | None = None,
               level: int | None = None, counts: torch.Tensor | None = None,
               gated: bool = True) -> GridIndex | None:
    """Cell grid over index's sorted points (knn_grid.hip), or None (CPU, GRID=off).

    The level comes from the point counts (grid_level_for); whether the grid applies is
    decided ON THE DEVICE (GRID=auto: lsk_hip_grid_decide from the level census and the
    crowding sum — clustered or multi-scale data keeps the bucket-tree walk of knn_rows,
    which adapts to density): the k-NN launch queues both kernels and the device runs the
    chosen one. No host read, so the build is graph-capturable and a stream of sets never
    waits for the previous set's k-NN here. `gated=False` (a halo index: whether its grid
    serves is the local index's gate): no census, no gate."""
    n = index.n
    if GRID == "off" or n == 0 or not K.is_gpu(index.pts):
        return None
    g = level if level is not None else grid_level_for(density_n if density_n is not None else n, n)
    slots = K.grid_build(index.pts, skeys, n, index.box, g - 2)
    gate = None
    if GRID == "auto" and gated:
        if counts is None:
            counts = K.key_levels_dev(skeys[:n])
        sq = K.grid_sq_dev(slots)
        gate = K.grid_decide(counts, sq, n, g, GRID_CROWD, True)
        census = (counts, sq)
    else:
        census = None
    return GridIndex(slots, g - 2, index.box, gate=gate, census=census)


HEAVY_RUN = 4096  # sorted points sharing one 30-bit key that trigger a second-level key
# HIP-graph captures cannot ask the host whether a cell is over-full. REFINE_CAPTURE
# (set by the caller from an eager warmup on the same kind of data, see LAST_REFINED)
# captures the refinement with fixed, data-independent sizes; otherwise the capture
# records a device flag (CAPTURED_HEAVY) that says after a replay whether some cell
# would have needed it (results stay exact either way, only the speed differs).
REFINE_CAPTURE = False
LAST_REFINED = False
CAPTURED_HEAVY: list = []
# Under host_sync_free() (a stream of point sets) the eager over-full-cell check does not
# read its flag either: it is kept here like a captured one (results stay exact, an
# unrefined cell only costs speed) and the stream reports it once the sets are done.
_SYNC_FREE = [0]
DEFERRED_HEAVY: list = []
# What a stream of sets knows about over-full cells: the flags of its sync-free builds in
# flight (pinned host copy, event) and the last one known. The first set of a stream, and
# every set once a known flag says the data has over-full cells, takes the eager check
# (one host read: refining such a set costs ~55 ms at 5e6 mixed-scale points, leaving it
# unrefined ~105 s, profiles/r5_stream/heavy_ab_deferred.log, heavy_ab_learned.log); sets after a known clean one stay
# sync-free.
_HEAVY_PENDING: list = []
_HEAVY_KNOWN: list = [None]


class host_sync_free:
    """Context: index builds queue no host read (see DEFERRED_HEAVY)."""

    def __enter__(self):
        _SYNC_FREE[0] += 1
        return self

    def __exit__(self, *exc):
        _SYNC_FREE[0] -= 1
        return False


def new_heavy_stream() -> None:
    """A new stream of sets starts knowing nothing about over-full cells: its first set
    takes the eager check (SetStream.run). The DEFERRED_HEAVY report is kept."""
    _HEAVY_PENDING.clear()
    _HEAVY_KNOWN[0] = None


def deferred_heavy_cells(clear: bool = False) -> bool:
    """Whether a build under host_sync_free() met an over-full cell it did not refine."""
    hit = any(bool(f) for f in DEFERRED_HEAVY)
    if clear:
        DEFERRED_HEAVY.clear()
        _HEAVY_PENDING.clear()
        _HEAVY_KNOWN[0] = None
    return hit


def refine_heavy_cells(points: torch.Tensor, skeys: torch.Tensor, perm: torch.Tensor,
                       heavy: torch.Tensor | None = None) -> torch.Tensor:
    """Order inside over-full key cells (docs/ARCHITECTURE.md §2a).

    Keys have 10 bits per axis of the global cube, so a cluster much smaller than one
    cell (huge dynamic range, e.g. a dense core in a large box) shares a single key and
    its buckets all overlap: the k-NN walk cannot cull inside it. The points of every
    run of more than HEAVY_RUN equal keys are re-keyed on the curve of the run's own
    bounding box and re-sorted by (run, local key) with the same radix sort; only the
    order changes (results are exact in any order). Eager: one compare pass + one host
    sync, then work and memory proportional to the over-full runs only. Inside a HIP
    graph capture: see REFINE_CAPTURE. `heavy`: the flag computed already (key_census)."""
    global LAST_REFINED
    n = skeys.shape[0]
    if n <= HEAVY_RUN:
        return perm
    heavy_any = heavy[0] != 0 if heavy is not None else (skeys[HEAVY_RUN:] == skeys[:-HEAVY_RUN]).any()
    if K.is_gpu(skeys) and torch.cuda.is_current_stream_capturing():
        if REFINE_CAPTURE:
            return _refine_all_cells(points, skeys, perm)
        CAPTURED_HEAVY.append(heavy_any)
        return perm
    if _SYNC_FREE[0] and K.is_gpu(skeys):
        while _HEAVY_PENDING and _HEAVY_PENDING[0][1].query():  # flags that landed (no wait)
            _HEAVY_KNOWN[0] = int(_HEAVY_PENDING.pop(0)[0][0]) != 0
        if _HEAVY_KNOWN[0] is False:
            flag = torch.empty(1, dtype=torch.int32, pin_memory=True)
            flag.copy_(heavy_any.reshape(1).to(torch.int32), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            _HEAVY_PENDING.append((flag, ev))
            DEFERRED_HEAVY.append(heavy_any)
            del DEFERRED_HEAVY[:-1024]
            return perm
        # first set of the stream, or the data is known to have over-full cells: eager
        # (the host read waits for this stream's queue)
        _HEAVY_KNOWN[0] = bool(heavy_any)
        if not _HEAVY_KNOWN[0]:
            return perm
        LAST_REFINED = True
        return _refine_heavy_runs(points, skeys, perm)
    if not bool(heavy_any):
        return perm
    LAST_REFINED = True
    return _refine_heavy_runs(points, skeys, perm)


def _local_keys(p: torch.Tensor, seg: torch.Tensor, nseg: int) -> torch.Tensor:
    """30-bit curve keys of points p on the bounding box of their segment."""
    dev = p.device
    if K.is_gpu(p):
        lo, hi = K.segment_bounds(p, seg, nseg)
    else:
        idx3 = seg.long()[:, None].expand(-1, 3)
        lo = torch.full((nseg, 3), math.inf, device=dev).scatter_reduce(0, idx3, p, "amin")
        hi = torch.full((nseg, 3), -math.inf, device=dev).scatter_reduce(0, idx3, p, "amax")
    ext = hi - lo
    ext = torch.where(ext > 0, ext, torch.ones_like(ext))
    sl = seg.long()
    q = ((p - lo[sl]) / ext[sl]).clamp_(0.0, 1.0).contiguous()
    del sl
    del lo, hi, ext
    # unit cube, scale just under 1024 cells so q = 1 stays in the last cell
    # (filled on the device: a host-to-device copy is not allowed inside a graph capture)
    unit = torch.ones(8, dtype=torch.float32, device=dev)
    unit[0:3].zero_()
    unit[6:7].fill_(1023.5)
    k2, _ = K.morton(q, unit, with_iota=False)
    return k2


def _refine_heavy_runs(points, skeys, perm):
    """Eager refinement restricted to the over-full runs (m points): O(m) memory."""
    n = skeys.shape[0]
    dev = skeys.device
    brk = torch.ones(n, dtype=torch.bool, device=dev)
    brk[1:] = skeys[1:] != skeys[:-1]
    starts = torch.nonzero(brk).view(-1)
    ends = torch.cat([starts[1:], torch.tensor([n], dtype=starts.dtype, device=dev)])
    lens = ends - starts
    heavy = lens > HEAVY_RUN
    hs, hl = starts[heavy], lens[heavy]
    nh = int(hs.shape[0])
    m = int(hl.sum())
    first = torch.cumsum(hl, 0) - hl                                          # run offsets in [m]
    # run id of every position: a 1 at each run's first offset, prefix-summed (torch's
    # repeat_interleave gives each run one thread: 3.9 ms for one 1e7-point run)
    seg = torch.zeros(m, dtype=torch.int32, device=dev)
    seg[first[1:]] = 1
    seg = torch.cumsum(seg, 0, dtype=torch.int32)                              # [m]
    pos = hs[seg] + (torch.arange(m, device=dev) - first[seg])                # sorted positions
    del brk, starts, ends, lens, heavy
    src = perm[pos].long()
    k2 = _local_keys(points[src], seg, nh)
    loc = torch.arange(m, dtype=torch.int32, device=dev)
    _, o1 = K.sort_pairs(k2, loc, 30)  # by local key ...
    sbits = max(1, (nh - 1).bit_length())
    _, o2 = K.sort_pairs(seg[o1.long()], o1, sbits)  # ... then stably by run
    out = perm.clone()
    out[pos] = perm[pos[o2.long()]]
    return out


def _refine_all_cells(points, skeys, perm):
    """Graph-capturable refinement: every cell re-keyed, all sizes bounded by n (no host
    sync; ~100 B per point of temporaries — used only when an eager warmup refined)."""
    n = skeys.shape[0]
    dev = skeys.device
    brk = torch.ones(n, dtype=torch.bool, device=dev)
    brk[1:] = skeys[1:] != skeys[:-1]
    rid = (torch.cumsum(brk, 0, dtype=torch.int32) - 1).contiguous()
    del brk
    k2 = _local_keys(points[perm.long()], rid, n)
    pos = torch.arange(n, dtype=torch.int32, device=dev)
    _, o1 = K.sort_pairs(k2, pos, 30)
    rbits = max(1, (n - 1).bit_length())
    _, o2 = K.sort_pairs(rid[o1.long()], o1, rbits)
    return perm[o2.long()].contiguous()


def captured_heavy_cells(clear: bool = False) -> bool:
    """After a replay: whether a captured build met an over-full cell it did not refine."""
    hit = any(bool(f) for f in CAPTURED_HEAVY)
    if clear:
        CAPTURED_HEAVY.clear()
    return hit


def radius_hint2(box: torch.Tensor, n_total: int, k: int) -> float:
    """Uniform-density estimate of the k-th squared distance (only used for groups
    whose own extent is zero)."""
    b = box.detach().cpu().tolist()
    ext = [max(b[3 + a] - b[a], 0.0) for a in range(3)]
    if not all(math.isfinite(e) for e in ext) or n_total <= 0:
        return 1.0
    nz = [e for e in ext if e > 0]
    if not nz:
        return 1.0
    measure = math.prod(nz)
    dim = len(nz)
    rho = n_total / measure
    unit = {1: 2.0, 2: math.pi, 3: 4.0 * math.pi / 3.0}[dim]
    r = (k / (unit * rho)) ** (1.0 / dim)
    return float(r * r)


def radius_hint(box: torch.Tensor, n_total: int, k: int) -> float | torch.Tensor:
    """radius_hint2 without a host round trip: for a GPU box a 1-element device tensor
    computed by a kernel (the k-NN kernel reads it in place), else the host float. Keeps
    the single-rank pipeline free of device->host syncs (HIP-graph capturable)."""
    if K.is_gpu(box):
        return K.radius_hint(box, n_total, k)
    return radius_hint2(box, n_total, k)


def query(index: LocalIndex, cfg: KnnConfig, hint2: float | torch.Tensor = 0.0, extra: LocalIndex | None = None,
          groups: torch.Tensor | None = None, ngroups: int = 0, out: torch.Tensor | None = None,
          stats: KnnStats | None = None, qstatus: torch.Tensor | None = None,
          init_d2: torch.Tensor | None = None, final_out: torch.Tensor | None = None,
          keep_d2: bool = False, deferred: list | None = None,
          ngroups_dev: torch.Tensor | None = None, short_list: bool = False, chunks: int = 1) -> torch.Tensor:
    """k-th squared distance of every (or every listed group of) sorted query of
    `index` against index's tree (+ `extra`'s tree). Returns d2 in sorted order.

    With `final_out` the kernel also writes the final distances in input order
    (final_out[index.perm[q]], fused scatter); then the sorted d2 is only produced (and
    returned) when `keep_d2` or `out` is given, else final_out is returned.

    `deferred` (a list): the failure-word read (a host sync) is not done here but queued
    on the list; `settle(deferred)` does it later — the launch stays asynchronous, so the
    host can queue other work (the overlapped halo exchange) behind it.
    `ngroups_dev` (with `groups`): the list's length as an int32 [1] tensor (on the GPU it
    stays on the device; `ngroups` is then the launch's upper bound); `short_list`: that
    length is expected far below ngroups; `chunks`: the pass as that many launches
    (kernels.knn_gpu)."""
    n = index.n
    want_d2 = final_out is None or keep_d2 or out is not None
    if out is None and want_d2:
        out = torch.empty(n, dtype=torch.float32, device=index.device)
    if n == 0:
        return out if want_d2 else final_out
    if not K.is_gpu(index.pts):
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=index.device)
        pts = index.pts[:n]
        if extra is not None and extra.n > 0:
            pts = torch.cat([pts, extra.pts[:extra.n]])
        if groups is None:
            out.copy_(K.kth_cpu(pts, index.pts[:n], cfg.k, cfg.cut2))
            rows = None
            KERNELS_USED.add("cpu")
        else:
            if ngroups_dev is not None:
                ngroups = int(ngroups_dev.view(-1)[0])
            g = groups[:ngroups].to(torch.int64)
            rows = (g[:, None] * 64 + torch.arange(64)[None, :]).reshape(-1)
            rows = rows[rows < n]
            out[rows] = K.kth_cpu(pts, index.pts[:n][rows], cfg.k, cfg.cut2)
        if final_out is not None:
            if rows is None:
                K.scatter1(out, index.perm, final_out, finalize=True)
            else:
                final_out[index.perm[rows].to(torch.int64)] = K.finalize_distances(out[rows])
        return out if want_d2 else final_out
    trees = [index.tree()] + ([extra.tree()] if extra is not None and extra.n > 0 else [])
    raw = torch.zeros(32, dtype=torch.int64, device=index.device) if stats is not None else None
    kw = dict(groups=groups, ngroups=ngroups, seed=SEED_BUCKETS, init_d2=init_d2,
              out_perm=index.perm if final_out is not None else None, out_final=final_out,
              qrot=index.qrot if len(trees) == 1 else None)
    impl = KNN_IMPL
    # two grids: the halo re-query of a distributed run (the halo index has a grid of its
    # own, pipelines._halo_requery); the local index's gate still picks grid or rows
    if index.qrot is not None and len(trees) != 1:
        raise ValueError("query: an index built in a rotated frame serves its own points only (no extra tree)")
    two_grid = (impl == "rows" and index.grid is not None and len(trees) == 2 and extra.grid is not None
                and cfg.k <= K.ROWS_MAX_K)
    use_grid = two_grid or (impl == "rows" and index.grid is not None and len(trees) == 1
                            and init_d2 is None and cfg.k <= K.ROWS_MAX_K)
    if len(trees) == 1 and init_d2 is None:  # (a local pass, not a halo re-query)
        if use_grid and index.grid.gate is not None:
            GATES_SEEN.append(index.grid.gate)  # grid or rows: resolved by kernels_used()
            GRIDS_SEEN[:] = [index.grid]  # (the last one: debugging)
            del GATES_SEEN[:-1024]  # (reporting only: a long stream keeps the last sets)
        else:
            KERNELS_USED.add("grid" if use_grid else impl)
    fw = K.knn_gpu(index.pts, n, trees, cfg.k, cfg.cut2, hint2, out, stats=raw, qstatus=qstatus,
                   impl="grid" if use_grid else impl, debug_fail_mod=DEBUG_FAIL_MOD,
                   grid=index.grid.view() if use_grid else None, ngroups_dev=ngroups_dev,
                   expect_grid=GRID_EXPECT[0], short_list=short_list, chunks=chunks,
                   grid2=extra.grid.view()[:4] if two_grid else None, **kw)
    gate = index.grid.gate if use_grid else None
    def check() -> bool:
        # one 4-byte read: failures beyond the list capacity (pathological input) rerun
        # the whole query on the exact kernel (on the current stream; returns True then)
        nfail = fw.value()
        rerun = nfail > fw.cap
        if gate is not None:  # (staged with the failure word: no wait for later work)
            GRID_EXPECT[0] = bool(fw.gate_value(gate))
        if rerun:
            K.knn_gpu(index.pts, n, trees, cfg.k, cfg.cut2, hint2, out, impl="exact", ngroups_dev=ngroups_dev,
                      **kw)
        if stats is not None:
            stats.add_fallback(nfail)
            stats.add(raw)
        return rerun

    if torch.cuda.is_current_stream_capturing():
        slot = len(CAPTURED_FAIL_WORDS)
        if fw.count is not None and CAPTURE_PEAKS is not None and slot < CAPTURE_PEAKS.numel():
            fw.peak = CAPTURE_PEAKS[slot:slot + 1]
            torch.maximum(fw.peak, fw.count.to(torch.int64) & 0xFFFFFFFF, out=fw.peak)
        CAPTURED_FAIL_WORDS.append(fw)
        if stats is not None:
            stats.add(raw)
    elif fw.count is None:
        if stats is not None:
            stats.add(raw)
    elif deferred is not None:
        fw.stage(gate)  # the later read waits for this launch only
        deferred.append(check)
    else:
        check()
    return out if want_d2 else final_out


# k-NN kernels the whole-set passes of this process used ("grid", "rows", "exact"): the
# bench reports them next to its number. Passes whose kernel the device picks leave their
# gate in GATES_SEEN; kernels_used() reads them (a host read: after the timed region).
KERNELS_USED: set = set()
GATES_SEEN: list = []
GRIDS_SEEN: list = []


def kernels_used() -> list:
    used = set(KERNELS_USED)
    for gate in GATES_SEEN:
        used.add("grid" if int(gate.item()) else "rows")
    return sorted(used)


def reset_kernels_used() -> None:
    KERNELS_USED.clear()
    GATES_SEEN.clear()


def settle(deferred: list) -> bool:
    """Run the failure checks `query(..., deferred=...)` queued (in launch order). True
    when one of them queued a rerun (its output is rewritten behind the current stream's
    work: a copy of it queued earlier is stale)."""
    rerun = False
    while deferred:
        rerun = bool(deferred.pop(0)()) or rerun
    return rerun


def verify_captured_failures(clear: bool = False) -> int:
    """After replaying a captured graph: total backstop queries of the captured launches;
    raises if one overflowed its failure list (the graph's output is then incomplete)."""
    total = 0
    for fw in CAPTURED_FAIL_WORDS:
        v = fw.value()
        peak = getattr(fw, "peak", None)
        if peak is not None:
            v = max(v, int(peak.item()))  # the worst replay
        if v > fw.cap:
            raise RuntimeError(f"k-NN failure list overflow in a captured graph ({v} > {fw.cap}): "
                               "rerun eagerly")
        total += v
    if clear:
        CAPTURED_FAIL_WORDS.clear()
    return total


def knn_distances(points: torch.Tensor, k: int, max_radius: float = math.inf,
                  stats: KnnStats | None = None, period=None) -> torch.Tensor:
    """Distance from every point to its k-th nearest neighbour among `points`
    (itself counted), in input order — the single-rank reference output. Open-box only: a
    `period` raises ValueError ("not supported"; knn_query_distances(points, points, ...) takes
    one)."""
    if period is not None:
        raise ValueError("knn_distances: a period is not supported (knn_query_distances(points, points, k, "
                         "period=...) gives the periodic k-th distances)")
    cfg = KnnConfig(k=k, max_radius=max_radius)
    probe = FrameProbe(points, k)
    if FRAME_EARLY:  # the probe read before the build (a short host wait, no wasted build)
        frame = probe.result()
        index = build_index(points, grid=frame is None, frame=frame)
    else:  # read after the unrotated build: no host wait before it
        index = build_index(points, grid=True)
        frame = probe.result()
        if frame is not None:  # a tilted plane: rebuilt in its principal-axes frame
            index = build_index(points, frame=frame)
    hint2 = radius_hint(index.box, index.n, k)
    out = torch.empty(index.n, dtype=torch.float32, device=points.device)
    return query(index, cfg, hint2, stats=stats, final_out=out)


def bucket_keys(index: LocalIndex) -> torch.Tensor:
    """Curve key (in index.box) of the first point of every bucket of `index`, cached on it.
    Non-decreasing: the points are sorted by these keys, and refine_heavy_cells only
    reorders points that share a key."""
    if index.bkeys is None:
        heads = index.pts[:index.n][::K.BUCKET].contiguous()
        index.bkeys = K.morton(heads, index.box, with_iota=False)[0]
    return index.bkeys


def prepare_queries(index: LocalIndex, queries: torch.Tensor, locate: bool = True) -> tuple:
    """Foreign queries brought into `index`'s curve order: (qsorted [nq + PAD, 3], qperm int32
    [nq]: sorted position -> query row, qbucket int32 [ceil(nq / 64)]: the data bucket each
    group of 64 sorted queries lies in, or None without `locate`: a walk that starts at the
    root needs the curve order only). Keys are taken in the index's cube; queries outside it
    (NaN included) clamp to its faces."""
    nq = queries.shape[0]
    keys = K.morton(queries, index.box, with_iota=False)[0]
    skeys, qperm = K.sort_keys_iota(keys, 30)
    qsorted = K.gather3(queries, qperm, pad=K.PAD_POINTS)
    return qsorted, qperm, K.locate_groups(skeys, nq, bucket_keys(index)) if locate else None


def _check_foreign(what: str, index: LocalIndex, queries: torch.Tensor) -> torch.Tensor:
    """The foreign queries of the public function `what`, checked and contiguous."""
    if queries.dim() != 2 or queries.shape[1] != 3 or queries.dtype != torch.float32:
        raise ValueError(f"{what}: queries must be a float32 [nq, 3] tensor")
    if queries.device != index.device:
        raise ValueError(f"{what}: queries on {queries.device}, the index on {index.device}")
    if index.qrot is not None:
        raise ValueError(f"{what}: an index built in a rotated frame serves its own points only")
    return queries.contiguous()


def _input_order(index: LocalIndex) -> torch.Tensor:
    """The points of a CPU index in input order (index.pts is curve-sorted)."""
    n = index.n
    inv = torch.empty(n, dtype=torch.int64)
    inv[index.perm[:n].long()] = torch.arange(n, dtype=torch.int64)
    return index.pts[:n][inv]


def _cutoff_distances(shape: tuple, cut2: float, device: torch.device) -> torch.Tensor:
    """No candidate at all: float32 `shape`, every slot the finalised cutoff."""
    return K.finalize_distances(torch.full((math.prod(shape),), cut2, dtype=torch.float32, device=device)).view(shape)


def query_points(index: LocalIndex, queries: torch.Tensor, cfg: KnnConfig, stats: KnnStats | None = None,
                 out: torch.Tensor | None = None, qstatus: torch.Tensor | None = None, period=None,
                 max_pairs: int = 1 << 28, flagged: torch.Tensor | None = None) -> torch.Tensor:
    """Distance from every row of `queries` (float32 [nq, 3] on the index's device) to its
    k-th nearest point of `index` (build_index(points, grid=True)), in query order. Only the
    index's points are candidates: a query that coincides with one finds it at distance 0,
    and no query is a candidate for another. The cutoff and k > n behave as in `query`.
    An index built in a rotated frame serves its own points only. `qstatus` (int32 [nq],
    debugging): the kernels' per-query status words, in curve-sorted query order.
    period: one value L or (Lx, Ly, Lz), each > 0, inf = open axis: the distance of a pair is
    the minimum image of its difference (radius_counts states the arithmetic), with no bound on
    the radius: the k-th smallest periodic squared distance by its bits among those below the
    cutoff. Only queries whose open-box ball reaches a face pay for it: they run a periodic
    radius search of at most `max_pairs` pairs at a time (a single query with more raises
    ValueError). `stats` also receives periodic_flagged, periodic_pairs and radius_images;
    `flagged` (bool [nq], tests) the queries that took the periodic passes."""
    per = _knn_period("query_points", index, period)
    queries = _check_foreign("query_points", index, queries)
    nq, n = queries.shape[0], index.n
    if out is None:
        out = torch.empty(nq, dtype=torch.float32, device=index.device)
    if flagged is not None:
        flagged.fill_(False)
    if nq == 0:
        return out
    if not K.is_gpu(index.pts):
        d2 = K.kth_cpu(index.pts[:n], queries, cfg.k, cfg.cut2) if per is None else \
            K.kth_periodic_cpu(index.pts[:n], queries, cfg.k, cfg.cut2, per)
        out.copy_(K.finalize_distances(d2))
        KERNELS_USED.add("cpu")
        return out
    if n == 0:  # no candidate at all: every answer is the cutoff
        out.copy_(_cutoff_distances((nq,), cfg.cut2, index.device))
        return out
    if per is None or cfg.k > n:  # (k > n: the cutoff under any distance)
        _foreign_kth(index, queries, cfg, stats, out, qstatus)
        return out
    qsorted, qperm, d2 = _foreign_kth(index, queries, cfg, stats, out, qstatus, want_d2=True)
    _periodic_knn(index, per, cfg, qsorted, qperm, d2, out, None, None, stats, max_pairs, flagged)
    return out


def _knn_period(what: str, index: LocalIndex | None, period) -> tuple | None:
    """The checked period of a k-NN query (None: open box, also when every axis is open);
    ValueError for a bad period, or a finite one with an index built in a rotated frame or
    sorted by line keys."""
    if period is None:
        return None
    per = K.check_period(what, period)
    if all(math.isinf(v) for v in per):
        return None
    if index is not None and (index.qrot is not None or index.line):
        raise ValueError(f"{what}: a period is not supported for an index built in a rotated frame or sorted "
                         "by line keys")
    return per


# the device error word of the last periodic k-NN pass (tests: always 0)
LAST_PERIODIC_KNN_ERRORS = [0]


def _flagged_slices(what: str, index: LocalIndex, per: tuple, cfg: KnnConfig, qsorted: torch.Tensor,
                    d2: torch.Tensor, max_pairs: int, raw: torch.Tensor | None = None) -> tuple:
    """The flag and count passes of the periodic k-NN (knn_periodic.hip) over the open-box k-th
    squared distances d2 (sorted-query order), and the slicing of the flagged rows: (cutq, qlist,
    pairs, slices) with qlist the flagged sorted queries (int32, ascending), pairs their total
    count and slices a list of (qlist[a:b], offsets int64 [b - a + 1], total, longest), each the
    longest run of rows within max_pairs pairs (a single row with more raises ValueError). Two
    host reads: the list's length and the counts' prefix sum."""
    nq = d2.shape[0]
    tree = index.tree()
    cutq, flags = K.pknn_flag_gpu(tree, qsorted, nq, d2, cfg.cut2, per)
    KERNELS_USED.add("knn_periodic")
    qlist = torch.nonzero(flags).view(-1).int()  # (host read: the list's length)
    m = qlist.numel()
    if m == 0:
        return cutq, qlist, 0, []
    counts = K.pknn_count_gpu(tree, qsorted, nq, qlist, cutq, per, stats=raw)
    cum = torch.zeros(m + 1, dtype=torch.int64, device=index.device)
    torch.cumsum(counts, 0, dtype=torch.int64, out=cum[1:])
    hcum = cum.cpu()  # (host read: decides the slices)
    hcounts = hcum[1:] - hcum[:-1]
    if int(hcounts.max()) > max_pairs:
        raise ValueError(f"{what}: a query has {int(hcounts.max())} points within its open-box k-th "
                         f"distance, more than max_pairs = {max_pairs}; raise max_pairs")
    slices = []
    a = 0
    while a < m:
        # the longest run of rows from a within max_pairs pairs (at least one: checked above)
        b = int(torch.searchsorted(hcum, hcum[a] + max_pairs, right=True)) - 1
        b = max(a + 1, min(b, m))
        slices.append((qlist[a:b].contiguous(), (cum[a:b + 1] - cum[a]).contiguous(), int(hcum[b] - hcum[a]),
                       int(hcounts[a:b].max())))
        a = b
    return cutq, qlist, int(hcum[m]), slices


def _periodic_knn(index: LocalIndex, per: tuple, cfg: KnnConfig, qsorted: torch.Tensor, qperm: torch.Tensor,
                  d2: torch.Tensor, out: torch.Tensor, out_idx: torch.Tensor | None, out_dist: torch.Tensor | None,
                  stats: KnnStats | None, max_pairs: int, flagged: torch.Tensor | None) -> None:
    """Turns the open-box results of _foreign_kth (and of the collect pass) into the periodic
    ones (knn_periodic.hip): the open-box k-th squared distance d2 bounds the periodic one, so
    only queries whose ball of that radius reaches a non-zero image of the root box are flagged;
    they run a periodic radius search with that bound, in slices of at most max_pairs pairs,
    and the first k of each sorted row overwrite their entries of out / out_idx / out_dist."""
    nq = d2.shape[0]
    raw = torch.zeros(K.RADIUS_PERIODIC_STATS, dtype=torch.int64, device=index.device) if stats is not None else None
    LAST_PERIODIC_KNN_ERRORS[0] = 0
    cutq, qlist, pairs, slices = _flagged_slices("periodic k-NN", index, per, cfg, qsorted, d2, max_pairs, raw)
    if flagged is not None:
        flagged[qperm[qlist.long()].long()] = True
    if slices:
        err = torch.zeros(1, dtype=torch.int32, device=index.device)
        for ql, offsets, total, longest in slices:
            K.pknn_rows_gpu(index.tree(), index.perm, qsorted, nq, ql, cutq, per, offsets, total, longest, qperm, d2,
                            cfg.cut2, cfg.k, out, out_idx, out_dist, err)
        LAST_PERIODIC_KNN_ERRORS[0] = int(err.item()) & 0xFFFFFFFF
    if stats is not None:
        _add_stats(stats, _RADIUS_PERIODIC_STATS, raw)
        stats.counters["periodic_flagged"] = stats.counters.get("periodic_flagged", 0) + qlist.numel()
        stats.counters["periodic_pairs"] = stats.counters.get("periodic_pairs", 0) + pairs
    if LAST_PERIODIC_KNN_ERRORS[0]:
        raise NativeError(f"periodic k-NN: {LAST_PERIODIC_KNN_ERRORS[0]} rows were not filled to their count or held "
                          "fewer than k points within the open-box k-th distance (a bug: that distance bounds "
                          "the periodic one)")


def _foreign_kth(index: LocalIndex, queries: torch.Tensor, cfg: KnnConfig, stats: KnnStats | None,
                 out: torch.Tensor, qstatus: torch.Tensor | None = None, want_d2: bool = False) -> tuple:
    """The foreign-query k-th pass shared by query_points and query_neighbors (a GPU index
    with n >= 1, nq >= 1 contiguous queries): gate, failure list and backstop as in query();
    `out` [nq] receives the final distances in query order. Returns (qsorted, qperm, d2):
    the curve-sorted queries, sorted position -> query row, and (want_d2) the k-th squared
    distances in sorted order, else None."""
    nq, n = queries.shape[0], index.n
    qsorted, qperm, qbucket = prepare_queries(index, queries)
    hint2 = radius_hint(index.box, n, cfg.k)
    raw = torch.zeros(32, dtype=torch.int64, device=index.device) if stats is not None else None
    d2 = torch.empty(nq, dtype=torch.float32, device=index.device) if want_d2 else None
    trees = [index.tree()]
    kw = dict(seed=SEED_BUCKETS, out_perm=qperm, out_final=out, qbucket=qbucket)
    impl = KNN_IMPL
    use_grid = impl == "rows" and index.grid is not None and cfg.k <= K.ROWS_MAX_K
    if use_grid and index.grid.gate is not None:  # (the index's gate decides, as for its own points)
        GATES_SEEN.append(index.grid.gate)
        del GATES_SEEN[:-1024]
    else:
        KERNELS_USED.add("grid" if use_grid else impl)
    fw = K.knn_gpu(qsorted, nq, trees, cfg.k, cfg.cut2, hint2, d2, stats=raw, qstatus=qstatus,
                   impl="grid" if use_grid else impl, debug_fail_mod=DEBUG_FAIL_MOD,
                   grid=index.grid.view() if use_grid else None, expect_grid=GRID_EXPECT[0], **kw)
    if fw.count is not None:
        # as query()'s check: failures beyond the list's capacity rerun every query exactly
        nfail = fw.value()
        if use_grid and index.grid.gate is not None:
            GRID_EXPECT[0] = bool(fw.gate_value(index.grid.gate))
        if nfail > fw.cap:
            K.knn_gpu(qsorted, nq, trees, cfg.k, cfg.cut2, hint2, d2, impl="exact", **kw)
        if stats is not None:
            stats.add_fallback(nfail)
    if stats is not None:
        stats.add(raw)
    return qsorted, qperm, d2


def knn_query_distances(points: torch.Tensor, queries: torch.Tensor, k: int, max_radius: float = math.inf,
                        stats: KnnStats | None = None, period=None, max_pairs: int = 1 << 28,
                        flagged: torch.Tensor | None = None) -> torch.Tensor:
    """Distance from every row of `queries` to its k-th nearest neighbour among `points`
    (both float32 [*, 3] on one device), in query order. The index is built in the points'
    own frame (no rotated frame, no line keys), so queries off a planar set's plane work.
    period / max_pairs / flagged: see query_points."""
    if points.device != queries.device:
        raise ValueError(f"knn_query_distances: points on {points.device}, queries on {queries.device}")
    _knn_period("knn_query_distances", None, period)
    cfg = KnnConfig(k=k, max_radius=max_radius)
    if points.shape[0] == 0:  # nothing to index: every answer is the cutoff
        if flagged is not None:
            flagged.fill_(False)
        return _cutoff_distances((queries.shape[0],), cfg.cut2, queries.device)
    index = build_index(points, grid=True)
    return query_points(index, queries, cfg, stats=stats, period=period, max_pairs=max_pairs, flagged=flagged)


def query_neighbors(index: LocalIndex, queries: torch.Tensor, cfg: KnnConfig, stats: KnnStats | None = None,
                    out_idx: torch.Tensor | None = None, out_dist: torch.Tensor | None = None, period=None,
                    max_pairs: int = 1 << 28, flagged: torch.Tensor | None = None) -> tuple:
    """Neighbour lists: (idx int32 [nq, k], dist float32 [nq, k]) in query order — for every
    row of `queries` the ids (rows of the indexed array) and distances of its k nearest
    points of `index` within the cutoff, ascending by (distance, row): ties at any distance,
    the k-th included, go to the lowest rows, whatever the index's internal order. Unfilled
    slots (fewer than k points qualify) hold -1 and the value the k-th-distance API returns
    there; dist[:, k - 1] is query_points' output bit for bit. Same inputs and limits as
    query_points, and k <= K.NEIGHBORS_MAX_K. period / max_pairs / flagged as in query_points:
    the lists are the first k of { (pd2, row) : pd2 < cut2 } with pd2 the periodic squared
    distance, in the same order and with the same tie rule."""
    per = _knn_period("query_neighbors", index, period)
    queries = _check_foreign("query_neighbors", index, queries)
    k = cfg.k
    if k < 1:
        raise ValueError("query_neighbors: k must be at least 1")
    if k > K.NEIGHBORS_MAX_K:
        raise ValueError(f"query_neighbors: k = {k} exceeds {K.NEIGHBORS_MAX_K} neighbours per query; "
                         "query_points / knn_query_distances give the k-th distance for any k")
    nq, n = queries.shape[0], index.n
    if out_idx is None:
        out_idx = torch.empty((nq, k), dtype=torch.int32, device=index.device)
    if out_dist is None:
        out_dist = torch.empty((nq, k), dtype=torch.float32, device=index.device)
    for t, dt in ((out_idx, torch.int32), (out_dist, torch.float32)):
        if t.shape != (nq, k) or t.dtype != dt or not t.is_contiguous() or t.device != index.device:
            raise ValueError("query_neighbors: out_idx int32 / out_dist float32, contiguous [nq, k] on the index's device")
    if flagged is not None:
        flagged.fill_(False)
    if nq == 0:
        return out_idx, out_dist
    if not K.is_gpu(index.pts):
        # (ids are rows of the input array: the lists are taken over the points in input order)
        idx, d2 = K.knn_cpu(_input_order(index), queries, k, cfg.cut2) if per is None else \
            K.knn_periodic_cpu(_input_order(index), queries, k, cfg.cut2, per)
        out_idx.copy_(idx)
        out_dist.copy_(K.finalize_distances(d2.view(-1)).view(nq, k))
        KERNELS_USED.add("cpu")
        return out_idx, out_dist
    if n == 0:  # no candidate at all
        out_idx.fill_(-1)
        out_dist.copy_(_cutoff_distances((nq, k), cfg.cut2, index.device))
        return out_idx, out_dist
    kth = torch.empty(nq, dtype=torch.float32, device=index.device)
    qsorted, qperm, d2 = _foreign_kth(index, queries, cfg, stats, kth, want_d2=True)
    err = K.knn_neighbors_gpu(index.tree(), index.perm, qsorted, nq, d2, k, cfg.cut2, qperm, out_idx, out_dist)
    LAST_NEIGHBOR_ERRORS[0] = int(err.item()) & 0xFFFFFFFF
    if LAST_NEIGHBOR_ERRORS[0]:
        raise NativeError(f"query_neighbors: {LAST_NEIGHBOR_ERRORS[0]} queries were handed a k-th distance that is "
                          "not their k-th value (a bug in the k-th pass or the collect pass)")
    if per is not None:  # (k > n included: the unfilled lists hold periodic distances too)
        _periodic_knn(index, per, cfg, qsorted, qperm, d2, kth, out_idx, out_dist, stats, max_pairs, flagged)
    return out_idx, out_dist


# the device error word of the last query_neighbors collect pass (tests: always 0)
LAST_NEIGHBOR_ERRORS = [0]


def knn_query_neighbors(points: torch.Tensor, queries: torch.Tensor, k: int, max_radius: float = math.inf,
                        stats: KnnStats | None = None, period=None, max_pairs: int = 1 << 28,
                        flagged: torch.Tensor | None = None) -> tuple:
    """(idx int32 [nq, k], dist float32 [nq, k]): ids and distances of the k nearest rows of
    `points` for every row of `queries` (both float32 [*, 3] on one device), see
    query_neighbors (period / max_pairs / flagged too). The index is built once, in the
    points' own frame."""
    if points.device != queries.device:
        raise ValueError(f"knn_query_neighbors: points on {points.device}, queries on {queries.device}")
    _knn_period("knn_query_neighbors", None, period)
    cfg = KnnConfig(k=k, max_radius=max_radius)
    if k > K.NEIGHBORS_MAX_K:
        raise ValueError(f"knn_query_neighbors: k = {k} exceeds {K.NEIGHBORS_MAX_K} neighbours per query; "
                         "knn_query_distances gives the k-th distance for any k")
    if points.shape[0] == 0:  # nothing to index: every slot is unfilled
        nq = queries.shape[0]
        if flagged is not None:
            flagged.fill_(False)
        return (torch.full((nq, k), -1, dtype=torch.int32, device=queries.device),
                _cutoff_distances((nq, k), cfg.cut2, queries.device))
    index = build_index(points, grid=True)
    return query_neighbors(index, queries, cfg, stats=stats, period=period, max_pairs=max_pairs, flagged=flagged)


def knn_neighbors(points: torch.Tensor, k: int, max_radius: float = math.inf,
                  stats: KnnStats | None = None, period=None, max_pairs: int = 1 << 28,
                  flagged: torch.Tensor | None = None) -> tuple:
    """knn_query_neighbors with the points as their own queries: every point's list starts
    with a point at distance 0 (itself, or the lowest row among its exact copies)."""
    return knn_query_neighbors(points, points, k, max_radius, stats=stats, period=period, max_pairs=max_pairs,
                               flagged=flagged)


# ------------------------------------------------------------------ fixed-radius search
# the device error word of the last radius_neighbors fill pass (tests: always 0)
LAST_RADIUS_ERRORS = [0]


def _radius_cut2(what: str, radius: float, squared: bool = False) -> float:
    r = float(radius)
    if math.isnan(r) or r < 0.0:
        raise ValueError(f"{what}: radius must be >= 0 (got {radius})")
    return float(np.float32(r)) if squared else cut2_of(r)


_RADIUS_STATS = ("radius_evals", "radius_nodes", "radius_buckets", "radius_box_accepts")


def _add_stats(stats: KnnStats | None, names: tuple, raw: torch.Tensor | None) -> None:
    """Add the words of a kernel's raw stats tensor to stats.counters under `names` (no stats: nothing)."""
    if stats is None:
        return
    for nm, v in zip(names, raw.cpu().tolist()):
        stats.counters[nm] = stats.counters.get(nm, 0) + int(v)


def _empty_csr(nq: int, dev: torch.device) -> tuple:
    return (torch.zeros(nq + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
            torch.empty(0, dtype=torch.float32, device=dev))


# ---- variable radii: one per query (gather) or one per indexed point (scatter)
def _cut2_tensor(what: str, name: str, radii: torch.Tensor, count: int, device: torch.device,
                 squared: bool, upper: float | None = None) -> torch.Tensor:
    """The float32 [count] squared cutoffs of a radius tensor (`squared`: the tensor itself).
    Wrong type, shape or device, or an entry that is negative or NaN: ValueError (one small
    device reduction is read for the last). upper: the largest entry a period admits; an entry
    above it raises too, in the same reduction."""
    if not isinstance(radii, torch.Tensor) or radii.dtype != torch.float32 or radii.dim() != 1 \
            or radii.shape[0] != count:
        got = f"{radii.dtype} {tuple(radii.shape)}" if isinstance(radii, torch.Tensor) else type(radii).__name__
        raise ValueError(f"{what}: {name} must be a float32 [{count}] tensor (got {got})")
    if radii.device != device:
        raise ValueError(f"{what}: {name} on {radii.device}, the index on {device}")
    r = radii.contiguous()
    if upper is not None:
        if count and not bool(((r >= 0) & (r <= upper)).all()):
            raise ValueError(f"{what}: every entry of {name} must be >= 0, not NaN and at most half the "
                             f"period of every finite axis ({upper} here)")
    elif count and not bool((r >= 0).all()):  # (a NaN fails the comparison too)
        raise ValueError(f"{what}: every entry of {name} must be >= 0 and not NaN")
    return r if squared else r * r


@dataclass
class PointRadii:
    """Per-point radii prepared for one index (prepare_point_radii)."""
    index: LocalIndex
    cut2: torch.Tensor                  # float32 [n] squared cutoffs, rows of the indexed array
    cut2_sorted: torch.Tensor | None    # GPU index: the same in the index's curve order
    nodes: torch.Tensor | None          # GPU index: copy of index.nodes, lo.w = largest cut2 below the node


def prepare_point_radii(index: LocalIndex, point_radii: torch.Tensor, squared: bool = False) -> PointRadii:
    """Per-point radii (float32 [n] on the index's device, in the order of the indexed array's
    rows; `squared`: squared cutoffs) made ready for the point_radius_* searches over
    `index`: the cutoffs in curve order and a private copy of the node array annotated with
    the largest cutoff below every node. The index itself is not written. Every point_radius_*
    function that takes an index accepts the result in place of the tensor, so a caller that
    sends queries in chunks prepares the radii once."""
    return _prepared_radii(index, _cut2_tensor("prepare_point_radii", "point_radii", point_radii, index.n,
                                               index.device, squared))


def _prepared_radii(index: LocalIndex, cut2: torch.Tensor) -> PointRadii:
    """The PointRadii of checked squared cutoffs (rows of the indexed array)."""
    if not K.is_gpu(index.pts) or index.n == 0:
        return PointRadii(index, cut2, None, None)
    cut2_sorted = cut2[index.perm[:index.n].long()].contiguous()
    nodes = index.nodes.clone()
    K.tree_set_radii(nodes, index.n, cut2_sorted)
    return PointRadii(index, cut2, cut2_sorted, nodes)


def _point_radii(what: str, index: LocalIndex, point_radii, squared: bool) -> PointRadii:
    if isinstance(point_radii, PointRadii):
        if point_radii.index is not index:
            raise ValueError(f"{what}: the point radii were prepared for another index")
        return point_radii
    try:
        return prepare_point_radii(index, point_radii, squared)
    except ValueError as e:
        raise ValueError(str(e).replace("prepare_point_radii", what, 1)) from None


def _var_counts(what: str, index: LocalIndex, queries: torch.Tensor, qcut2: torch.Tensor | None,
                prad: PointRadii | None, stats: KnnStats | None, _sorted: tuple | None = None) -> torch.Tensor:
    """radius_counts with cutoffs per query (qcut2) or per point (prad); checked arguments."""
    nq, n = queries.shape[0], index.n
    if nq == 0 or n == 0:
        return torch.zeros(nq, dtype=torch.int32, device=index.device)
    if not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        if prad is None:
            return K.radius_var_count_cpu(index.pts[:n], queries, qcut2, None)
        return K.radius_var_count_cpu(_input_order(index), queries, None, prad.cut2)
    qsorted, qperm = _sorted if _sorted is not None else prepare_queries(index, queries, locate=False)[:2]
    raw = torch.zeros(4, dtype=torch.int64, device=index.device) if stats is not None else None
    if prad is None:
        counts = K.radius_var_count_gpu(index.tree(), qsorted, nq, qperm, qcut2=qcut2, stats=raw)
    else:
        tree = (index.pts, prad.nodes, index.qnodes, n, index.depth)
        counts = K.radius_var_count_gpu(tree, qsorted, nq, qperm, pcut2=prad.cut2_sorted, stats=raw)
    KERNELS_USED.add("radius_var")
    _add_stats(stats, _RADIUS_STATS, raw)
    return counts


def _var_neighbors(what: str, index: LocalIndex, queries: torch.Tensor, qcut2: torch.Tensor | None,
                   prad: PointRadii | None, sort: bool, max_pairs: int) -> tuple:
    """radius_neighbors with cutoffs per query (qcut2) or per point (prad); checked arguments."""
    nq, n = queries.shape[0], index.n
    dev = index.device
    gpu = K.is_gpu(index.pts)
    if nq == 0 or n == 0:
        return _empty_csr(nq, dev)
    prep = prepare_queries(index, queries, locate=False)[:2] if gpu else None
    counts = _var_counts(what, index, queries, qcut2, prad, None, _sorted=prep)
    offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    total, longest = (int(v) for v in torch.stack((offsets[nq], counts.max().long())).tolist())  # the only sync
    if total > max_pairs:
        raise ValueError(f"{what}: {total} pairs within the radii exceed max_pairs = {max_pairs}; "
                         "query fewer points at a time or raise max_pairs")
    if not gpu:
        o2, idx, d2 = K.radius_var_cpu(_input_order(index), queries, qcut2, None if prad is None else prad.cut2)
        return o2, idx, K.finalize_distances(d2)
    qsorted, qperm = prep
    if prad is None:
        idx, dist, err = K.radius_var_fill_gpu(index.tree(), index.perm, qsorted, nq, qperm, offsets, total, longest,
                                               qcut2=qcut2, sort=sort)
    else:
        tree = (index.pts, prad.nodes, index.qnodes, n, index.depth)
        idx, dist, err = K.radius_var_fill_gpu(tree, index.perm, qsorted, nq, qperm, offsets, total, longest,
                                               pcut2=prad.cut2_sorted, sort=sort)
    LAST_RADIUS_ERRORS[0] = int(err.item()) & 0xFFFFFFFF
    if LAST_RADIUS_ERRORS[0]:
        raise NativeError(f"{what}: {LAST_RADIUS_ERRORS[0]} rows were not filled to their count "
                          "(the count pass and the fill pass disagree: a bug)")
    return offsets, idx, dist


# ---- periodic box: the minimum image of the difference (periodic.hip)
def wrap_points(points: torch.Tensor, period, origin=0.0) -> torch.Tensor:
    """`points` (float32 [n, 3]) brought into one period: on every finite axis the result lies in
    [origin, origin + L), also after rounding, and wrapping it again changes nothing; open axes
    (L = inf) and NaN or infinite coordinates pass through. period / origin: one value or three.
    The periodic searches take any finite input (a single wrap per axis, literally); for
    coordinates inside one period their distance is the physical periodic one."""
    per = K.check_period("wrap_points", period)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("wrap_points: points must be a float32 [n, 3] tensor")
    org = (origin,) * 3 if isinstance(origin, (int, float)) else tuple(origin)
    if len(org) != 3 or not all(math.isfinite(float(o)) for o in org):
        raise ValueError("wrap_points: origin must be one finite value or three")
    out = points.clone()
    for a in range(3):
        if not math.isfinite(per[a]):
            continue
        L, o = float(per[a]), float(np.float32(org[a]))
        hi = float(np.float32(o) + np.float32(L))  # fl(origin + L): the first value no longer inside
        x = out[:, a]
        # float64 holds x - origin and the multiple of L without a visible error; what rounding to
        # float32 (or the floor's own last bit) leaves on or past an edge is the lower edge itself
        y = x.double()
        w = (y - torch.floor((y - o) / L) * L).float()
        w = torch.where((w >= hi) | (w < o), torch.full_like(w, o), w)
        out[:, a] = torch.where(torch.isfinite(x), w, x)
    return out


def period_radius_bound(per: tuple, squared: bool) -> float:
    """The largest radius (squared: squared cutoff) the period `per` admits: fl(0.5 L) (squared:
    fl(h h)) of its shortest finite axis, inf when every axis is open."""
    finite = [np.float32(0.5) * np.float32(v) for v in per if math.isfinite(v)]
    if not finite:
        return math.inf
    return K.period_cut2_bound(per) if squared else float(min(finite))


def check_period_radius(what: str, radius: float, squared: bool, period, name: str = "radius") -> tuple:
    """The checked period values of a search with one radius; ValueError for a bad period or a
    radius above period_radius_bound."""
    per = K.check_period(what, period)
    upper = period_radius_bound(per, squared)
    if float(np.float32(radius)) > upper:
        raise ValueError(f"{what}: {name} {radius} exceeds half the period of a finite axis "
                         f"({'squared ' if squared else ''}bound {upper})")
    return per


def _period_cutoffs(what: str, index: LocalIndex, queries: torch.Tensor, radius, squared: bool, period) -> tuple:
    """The checked arguments of a periodic radius search: (period values, queries, cut2, qcut2).
    The radius, one value or one per query, may not exceed half the period of a finite axis (r
    <= fl(0.5 L); squared: cut2 <= fl(h h)): ValueError before any kernel runs, for a tensor in
    the one reduction that checks its entries."""
    per = K.check_period(what, period)
    queries = _check_foreign(what, index, queries)
    if isinstance(radius, torch.Tensor):
        upper = period_radius_bound(per, squared)
        qcut2 = _cut2_tensor(what, "radius", radius, queries.shape[0], index.device, squared,
                             upper=None if math.isinf(upper) else upper)
        return per, queries, 0.0, qcut2
    cut2 = _radius_cut2(what, radius, squared)
    check_period_radius(what, radius, squared, per)
    return per, queries, cut2, None


_RADIUS_PERIODIC_STATS = _RADIUS_STATS + ("radius_images",)


def _periodic_counts(index: LocalIndex, queries: torch.Tensor, cut2: float, qcut2: torch.Tensor | None,
                     per: tuple, stats: KnnStats | None, _sorted: tuple | None = None) -> torch.Tensor:
    nq, n = queries.shape[0], index.n
    if nq == 0 or n == 0:
        return torch.zeros(nq, dtype=torch.int32, device=index.device)
    if not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        return K.radius_periodic_count_cpu(index.pts[:n], queries, cut2, per, qcut2)
    qsorted, qperm = _sorted if _sorted is not None else prepare_queries(index, queries, locate=False)[:2]
    raw = torch.zeros(K.RADIUS_PERIODIC_STATS, dtype=torch.int64, device=index.device) if stats is not None else None
    counts = K.radius_periodic_count_gpu(index.tree(), qsorted, nq, cut2, qperm, per, qcut2=qcut2, stats=raw)
    KERNELS_USED.add("radius_periodic")
    _add_stats(stats, _RADIUS_PERIODIC_STATS, raw)
    return counts


def _periodic_neighbors(what: str, index: LocalIndex, queries: torch.Tensor, cut2: float,
                        qcut2: torch.Tensor | None, per: tuple, sort: bool, max_pairs: int) -> tuple:
    nq, n = queries.shape[0], index.n
    dev = index.device
    gpu = K.is_gpu(index.pts)
    if nq == 0 or n == 0:
        return _empty_csr(nq, dev)
    prep = prepare_queries(index, queries, locate=False)[:2] if gpu else None
    counts = _periodic_counts(index, queries, cut2, qcut2, per, None, _sorted=prep)
    offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    total, longest = (int(v) for v in torch.stack((offsets[nq], counts.max().long())).tolist())  # the only sync
    if total > max_pairs:
        raise ValueError(f"{what}: {total} pairs within the radius exceed max_pairs = {max_pairs}; "
                         "query fewer points at a time or raise max_pairs")
    if not gpu:
        o2, idx, d2 = K.radius_periodic_cpu(_input_order(index), queries, cut2, per, qcut2)
        return o2, idx, K.finalize_distances(d2)
    qsorted, qperm = prep
    idx, dist, err = K.radius_periodic_fill_gpu(index.tree(), index.perm, qsorted, nq, cut2, qperm, offsets, total,
                                                longest, per, qcut2=qcut2, sort=sort)
    LAST_RADIUS_ERRORS[0] = int(err.item()) & 0xFFFFFFFF
    if LAST_RADIUS_ERRORS[0]:
        raise NativeError(f"{what}: {LAST_RADIUS_ERRORS[0]} rows were not filled to their count "
                          "(the count pass and the fill pass disagree: a bug)")
    return offsets, idx, dist


def radius_counts(index: LocalIndex, queries: torch.Tensor, radius: float | torch.Tensor,
                  stats: KnnStats | None = None, _sorted: tuple | None = None, squared: bool = False,
                  period=None) -> torch.Tensor:
    """int32 [nq], in query order: for every row of `queries` (float32 [nq, 3] on the index's
    device) the number of points of `index` with dist2(q, p) < cut2_of(radius) — the strict
    comparison of the k-th-distance cutoff, so count >= k exactly when query_points with that
    k and max_radius = radius answers below the cutoff value. radius = 0 counts nothing,
    radius = inf every point; a query with a NaN or infinite coordinate counts nothing. Boxes
    that lie wholly inside a query's ball are counted without visiting their points, so large
    radii cost far less than n distance evaluations per query. `stats` receives
    radius_evals / radius_nodes / radius_buckets / radius_box_accepts.

    `radius` may be a float32 tensor [nq] on the index's device, one radius per query row
    (gather: p counts for q iff dist2(q, p) < cut2[q]); a negative or NaN entry raises
    ValueError before any kernel runs. squared=True: the given value(s) are the squared
    cutoffs themselves (the engine's own squared distances can be handed back as they are).

    period: one value L or (Lx, Ly, Lz), each > 0, inf = open axis: the box is periodic and
    dist2 becomes the minimum image of the difference — per axis, in float32, d = q - p; d >
    L/2: d - L; d < -L/2: d + L — so the distance is symmetric in its bits and a pair belongs to
    one image. It is the physical periodic distance for coordinates inside one period
    (wrap_points brings them there); no origin enters it. The radius (every entry) may not
    exceed half the period of a finite axis: ValueError before any kernel runs, as for a bad
    period. `stats` also receives radius_images, the image walks summed over the query groups.
    None: the open box, the path without this argument."""
    if period is not None:
        per, queries, cut2, qcut2 = _period_cutoffs("radius_counts", index, queries, radius, squared, period)
        return _periodic_counts(index, queries, cut2, qcut2, per, stats, _sorted=_sorted)
    if isinstance(radius, torch.Tensor):
        queries = _check_foreign("radius_counts", index, queries)
        qcut2 = _cut2_tensor("radius_counts", "radius", radius, queries.shape[0], index.device, squared)
        return _var_counts("radius_counts", index, queries, qcut2, None, stats, _sorted=_sorted)
    cut2 = _radius_cut2("radius_counts", radius, squared)
    queries = _check_foreign("radius_counts", index, queries)
    nq, n = queries.shape[0], index.n
    if nq == 0 or n == 0:
        return torch.zeros(nq, dtype=torch.int32, device=index.device)
    if not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        return K.radius_count_cpu(index.pts[:n], queries, cut2)
    qsorted, qperm = _sorted if _sorted is not None else prepare_queries(index, queries, locate=False)[:2]
    raw = torch.zeros(4, dtype=torch.int64, device=index.device) if stats is not None else None
    counts = K.radius_count_gpu(index.tree(), qsorted, nq, cut2, qperm, stats=raw)
    KERNELS_USED.add("radius")
    _add_stats(stats, _RADIUS_STATS, raw)
    return counts


def radius_neighbors(index: LocalIndex, queries: torch.Tensor, radius: float | torch.Tensor, sort: bool = True,
                     max_pairs: int = 1 << 28, squared: bool = False, period=None) -> tuple:
    """Fixed-radius neighbour lists in CSR form, in query order: (offsets int64 [nq + 1], idx
    int32 [total], dist float32 [total]). Row q = [offsets[q], offsets[q + 1]) holds every
    point of `index` with dist2(q, p) < cut2_of(radius) (see radius_counts), however many
    there are: idx are rows of the indexed array, dist the final distances. sort=True: each
    row ascending by (dist2 bits, row), the order of the neighbour lists, whatever the
    index's internal order; sort=False: unspecified order inside a row (cheaper). More than
    `max_pairs` pairs in all raise ValueError before anything is allocated for them.
    `radius` may be a float32 tensor [nq], one radius per query row; `squared` and `period`
    as in radius_counts (under a period dist holds the periodic distances)."""
    if period is not None:
        per, queries, cut2, qcut2 = _period_cutoffs("radius_neighbors", index, queries, radius, squared, period)
        return _periodic_neighbors("radius_neighbors", index, queries, cut2, qcut2, per, sort, max_pairs)
    if isinstance(radius, torch.Tensor):
        queries = _check_foreign("radius_neighbors", index, queries)
        qcut2 = _cut2_tensor("radius_neighbors", "radius", radius, queries.shape[0], index.device, squared)
        return _var_neighbors("radius_neighbors", index, queries, qcut2, None, sort, max_pairs)
    cut2 = _radius_cut2("radius_neighbors", radius, squared)
    queries = _check_foreign("radius_neighbors", index, queries)
    nq, n = queries.shape[0], index.n
    dev = index.device
    gpu = K.is_gpu(index.pts)
    if nq == 0 or n == 0:
        return _empty_csr(nq, dev)
    prep = prepare_queries(index, queries, locate=False)[:2] if gpu else None
    counts = radius_counts(index, queries, radius, _sorted=prep, squared=squared)
    offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    total, longest = (int(v) for v in torch.stack((offsets[nq], counts.max().long())).tolist())  # the only sync
    if total > max_pairs:
        raise ValueError(f"radius_neighbors: {total} pairs within the radius exceed max_pairs = {max_pairs}; "
                         "query fewer points at a time or raise max_pairs")
    if not gpu:
        o2, idx, d2 = K.radius_cpu(_input_order(index), queries, cut2)
        return o2, idx, K.finalize_distances(d2)
    qsorted, qperm = prep
    idx, dist, err = K.radius_fill_gpu(index.tree(), index.perm, qsorted, nq, cut2, qperm, offsets, total, longest,
                                       sort=sort)
    LAST_RADIUS_ERRORS[0] = int(err.item()) & 0xFFFFFFFF
    if LAST_RADIUS_ERRORS[0]:
        raise NativeError(f"radius_neighbors: {LAST_RADIUS_ERRORS[0]} rows were not filled to their count "
                          "(the count pass and the fill pass disagree: a bug)")
    return offsets, idx, dist


def _check_radius(what: str, radius, nq: int, device: torch.device, squared: bool) -> None:
    """The checks of a scalar or per-query radius where nothing is searched (no points)."""
    if isinstance(radius, torch.Tensor):
        _cut2_tensor(what, "radius", radius, nq, device, squared)
    else:
        _radius_cut2(what, radius, squared)


def radius_query_counts(points: torch.Tensor, queries: torch.Tensor, radius: float | torch.Tensor,
                        stats: KnnStats | None = None, squared: bool = False, period=None) -> torch.Tensor:
    """radius_counts over an index built once from `points` (both float32 [*, 3] on one
    device), in the points' own frame."""
    if points.device != queries.device:
        raise ValueError(f"radius_query_counts: points on {points.device}, queries on {queries.device}")
    if points.shape[0] == 0:  # nothing to index
        if period is not None:
            K.check_period("radius_query_counts", period)
        _check_radius("radius_query_counts", radius, queries.shape[0], queries.device, squared)
        return torch.zeros(queries.shape[0], dtype=torch.int32, device=queries.device)
    if period is not None:
        return radius_counts(build_index(points), queries, radius, stats=stats, squared=squared, period=period)
    return radius_counts(build_index(points), queries, radius, stats=stats, squared=squared)


def radius_query_neighbors(points: torch.Tensor, queries: torch.Tensor, radius: float | torch.Tensor,
                           sort: bool = True, max_pairs: int = 1 << 28, squared: bool = False,
                           period=None) -> tuple:
    """radius_neighbors over an index built once from `points`, in the points' own frame."""
    if points.device != queries.device:
        raise ValueError(f"radius_query_neighbors: points on {points.device}, queries on {queries.device}")
    if points.shape[0] == 0:  # nothing to index: every row is empty
        if period is not None:
            K.check_period("radius_query_neighbors", period)
        _check_radius("radius_query_neighbors", radius, queries.shape[0], queries.device, squared)
        return _empty_csr(queries.shape[0], queries.device)
    if period is not None:
        return radius_neighbors(build_index(points), queries, radius, sort=sort, max_pairs=max_pairs,
                                squared=squared, period=period)
    return radius_neighbors(build_index(points), queries, radius, sort=sort, max_pairs=max_pairs, squared=squared)


def radius_self_neighbors(points: torch.Tensor, radius: float | torch.Tensor, sort: bool = True,
                          max_pairs: int = 1 << 28, squared: bool = False, period=None) -> tuple:
    """radius_query_neighbors with the points as their own queries: for radius > 0 every
    sorted row starts with a point at distance 0 (itself, or the lowest row among its
    exact copies)."""
    return radius_query_neighbors(points, points, radius, sort=sort, max_pairs=max_pairs, squared=squared,
                                  period=period)


# ---- radius profiles: counts at many radii from one walk (radius_profile.hip)
def _profile_cutoffs(what: str, radii, squared: bool, period) -> tuple:
    """The checked radii of a profile: (cut2s float32 CPU tensor [B], period values or None).
    ValueError for no radius, a negative or NaN one, radii that do not ascend, a bad period or
    a radius above the period's bound; nothing on a device is read."""
    if isinstance(radii, torch.Tensor):
        if radii.device.type != "cpu" or radii.dtype not in (torch.float32, torch.float64) or radii.dim() != 1:
            raise ValueError(f"{what}: radii must be a sequence or a float32 / float64 CPU tensor [B] "
                             f"(got {radii.dtype} {tuple(radii.shape)} on {radii.device})")
        vals = radii.tolist()
    else:
        try:
            vals = [float(r) for r in radii]
        except (TypeError, ValueError):
            raise ValueError(f"{what}: radii must be a sequence of numbers or a CPU tensor") from None
    if not vals:
        raise ValueError(f"{what}: radii must hold at least one radius")
    per = None if period is None else K.check_period(what, period)
    for r in vals:
        _radius_cut2(what, r, squared)
        if per is not None:
            check_period_radius(what, r, squared, per)
    if any(b < a for a, b in zip(vals, vals[1:])):
        raise ValueError(f"{what}: radii must ascend (got {vals})")
    return torch.tensor([_radius_cut2(what, r, squared) for r in vals], dtype=torch.float32), per


def _profile(what: str, index: LocalIndex, queries: torch.Tensor, radii, squared: bool, period,
             stats: KnnStats | None, sums: bool, weights: tuple | None = None) -> torch.Tensor:
    """The runner of the radius profiles. sums: the [B] sums over the queries in the place of the [nq,
    B] profile; weights: None = the counts, else (point weights, query weights or None) of the
    weighted forms (query weights belong to the sums alone)."""
    cut2s, per = _profile_cutoffs(what, radii, squared, period)
    if index.qrot is not None or index.line:
        raise ValueError(f"{what}: an index built in a rotated frame or sorted by line keys is not supported")
    queries = _check_foreign(what, index, queries)
    nq, n, nb = queries.shape[0], index.n, cut2s.shape[0]
    pw = wq = None
    if weights is not None:
        pw = _point_weights(what, index, weights[0])
        if sums:
            if weights[1] is not None:
                wq = K.int64_weights(what, "query_weights", weights[1], nq, index.device)
            check_pair_sum_bound(what, pw, wq, nq)
    if nq == 0 or n == 0:
        return torch.zeros(nb if sums else (nq, nb), dtype=torch.int64 if sums or weights is not None else torch.int32,
                           device=index.device)
    if not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        if weights is None:
            return (K.pair_counts_cpu if sums else K.radius_profile_cpu)(index.pts[:n], queries, cut2s, per)
        if sums:
            return K.weighted_pair_sums_cpu(index.pts[:n], queries, cut2s, pw.sorted, per, query_weights=wq)
        return K.weighted_profile_cpu(index.pts[:n], queries, cut2s, pw.sorted, per)
    qsorted, qperm = prepare_queries(index, queries, locate=False)[:2]
    names = _RADIUS_STATS if per is None else _RADIUS_PERIODIC_STATS
    raw = torch.zeros(len(names), dtype=torch.int64, device=index.device) if stats is not None else None
    if weights is None:
        out = (K.pair_counts_gpu if sums else K.radius_profile_gpu)(index.tree(), qsorted, nq, cut2s, qperm, per,
                                                                    stats=raw)
    elif sums:
        out = K.weighted_pair_sums_gpu(index.tree(), qsorted, nq, cut2s, qperm, pw.sorted, pw.prefix,
                                       query_weights=wq, period=per, stats=raw)
    else:
        out = K.weighted_profile_gpu(index.tree(), qsorted, nq, cut2s, qperm, pw.sorted, pw.prefix, period=per,
                                     stats=raw)
    KERNELS_USED.add("radius_profile" if weights is None else "weighted_profile")
    _add_stats(stats, names, raw)
    return out


def radius_profile(index: LocalIndex, queries: torch.Tensor, radii, squared: bool = False, period=None,
                   stats: KnnStats | None = None) -> torch.Tensor:
    """int32 [nq, B], in query order: P[q, b] = the number of points of `index` with dist2(q, p)
    < cut2_of(radii[b]), strict and cumulative, for B >= 1 ascending radii from one walk of the
    tree. Column b equals radius_counts(index, queries, radii[b], squared=..., period=...) bit
    for bit: that is the whole definition; the counts in the shell between two radii are P[:,
    b] - P[:, b - 1]. radii: a Python sequence or a float32 / float64 CPU tensor, each >= 0,
    inf and duplicates allowed; squared=True: the squared cutoffs themselves. With `period`
    dist2 is the minimum image of radius_counts and every radius must respect its bound (half
    the period of a finite axis). A query with a NaN or infinite coordinate counts nothing in
    every column. Limit inherited from radius_counts: whole boxes are counted without visiting
    their points, which is exact for finite indexed points; an *indexed* point with a NaN
    coordinate is invisible to the tree's boxes, so a box that is accepted whole counts it
    (and the two functions need not accept the same boxes: the column identity holds for
    finite indexed points).

    No radius, a negative or NaN radius, radii that do not ascend, a radius above the period's
    bound and the failures of radius_counts' own argument checks raise ValueError before any
    kernel runs, without a device read. An index built in a rotated frame or sorted by line
    keys is not supported. `stats` receives radius_evals / radius_nodes / radius_buckets /
    radius_box_accepts, and radius_images under a period. More than 32 radii are served in
    slices of 32, one walk each."""
    return _profile("radius_profile", index, queries, radii, squared, period, stats, False)


def pair_counts(index: LocalIndex, queries: torch.Tensor, radii, squared: bool = False, period=None,
                stats: KnnStats | None = None) -> torch.Tensor:
    """int64 [B] on the index's device: S[b] = the sum over all queries of radius_profile's P[q,
    b], the cumulative pair counts DR(< r_b) of a two-point histogram (shell b holds S[b] - S[b
    - 1] pairs), without ever allocating anything of size nq x B. Integer sums: two runs give
    the same bits. Arguments and errors as for radius_profile."""
    return _profile("pair_counts", index, queries, radii, squared, period, stats, True)


def _profile_index(what: str, points: torch.Tensor, queries: torch.Tensor, radii, squared: bool, period,
                   weights: tuple | None = None) -> LocalIndex | None:
    """The index of the *_query_* / *_self_* profile forms; None when there is nothing to index (the
    radii, and the (point weights, query weights or None) of a weighted form, are checked all the
    same)."""
    if points.device != queries.device:
        raise ValueError(f"{what}: points on {points.device}, queries on {queries.device}")
    if points.shape[0] == 0:
        _profile_cutoffs(what, radii, squared, period)
        if weights is not None:
            K.int64_weights(what, "weights", weights[0], 0, points.device)
            if weights[1] is not None:
                K.int64_weights(what, "query_weights", weights[1], queries.shape[0], queries.device)
        return None
    return build_index(points)


def radius_query_profile(points: torch.Tensor, queries: torch.Tensor, radii, squared: bool = False, period=None,
                         stats: KnnStats | None = None) -> torch.Tensor:
    """radius_profile over an index built once from `points` (both float32 [*, 3] on one
    device), in the points' own frame."""
    index = _profile_index("radius_query_profile", points, queries, radii, squared, period)
    if index is None:
        return torch.zeros((queries.shape[0], len(radii)), dtype=torch.int32, device=queries.device)
    return radius_profile(index, queries, radii, squared=squared, period=period, stats=stats)


def radius_self_profile(points: torch.Tensor, radii, squared: bool = False, period=None,
                        stats: KnnStats | None = None) -> torch.Tensor:
    """radius_query_profile with the points as their own queries: every finite point counts
    itself (and its exact copies) at every radius > 0."""
    return radius_query_profile(points, points, radii, squared=squared, period=period, stats=stats)


def pair_query_counts(points: torch.Tensor, queries: torch.Tensor, radii, squared: bool = False, period=None,
                      stats: KnnStats | None = None) -> torch.Tensor:
    """pair_counts over an index built once from `points`, in the points' own frame."""
    index = _profile_index("pair_query_counts", points, queries, radii, squared, period)
    if index is None:
        return torch.zeros(len(radii), dtype=torch.int64, device=queries.device)
    return pair_counts(index, queries, radii, squared=squared, period=period, stats=stats)


def pair_self_counts(points: torch.Tensor, radii, squared: bool = False, period=None,
                     stats: KnnStats | None = None) -> torch.Tensor:
    """pair_query_counts with the points as their own queries. S[b] counts ordered pairs, (p, q)
    and (q, p) both, and every finite point with itself (at every radius > 0). The unordered
    pair count of a DD histogram is the caller's step, not the library's: DD_unordered = (S -
    S_at_zero_distance) / 2, where S_at_zero_distance is the count at the smallest radius above
    0 that separates nothing but exact copies (n for a set without duplicates)."""
    return pair_query_counts(points, points, radii, squared=squared, period=period, stats=stats)


# ---- anisotropic pair counts: DD(rp, pi) and DD(s, mu) along a box axis or an observer's line
# of sight (pair_counts_2d.hip)
_LOS = {"x": 0, "y": 1, "z": 2}


def _edge_values(what: str, name: str, edges) -> list:
    """The numbers of one list of bin edges (a sequence or a float32 / float64 CPU tensor [B], 1 <=
    B <= 2048), each >= 0 and not NaN, ascending; nothing on a device is read."""
    if isinstance(edges, torch.Tensor):
        if edges.device.type != "cpu" or edges.dtype not in (torch.float32, torch.float64) or edges.dim() != 1:
            raise ValueError(f"{what}: {name} must be a sequence or a float32 / float64 CPU tensor [B] "
                             f"(got {edges.dtype} {tuple(edges.shape)} on {edges.device})")
        vals = edges.tolist()
    else:
        try:
            vals = [float(r) for r in edges]
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {name} must be a sequence of numbers or a CPU tensor") from None
    if not 1 <= len(vals) <= K.PAIRS2D_MAX_EDGES:
        raise ValueError(f"{what}: {name} must hold 1 .. {K.PAIRS2D_MAX_EDGES} values (got {len(vals)})")
    if any(math.isnan(v) or v < 0.0 for v in vals):
        raise ValueError(f"{what}: every value of {name} must be >= 0 (got {vals})")
    if any(b < a for a, b in zip(vals, vals[1:])):
        raise ValueError(f"{what}: {name} must ascend (got {vals})")
    return vals


def _pairs2d_cutoffs(what: str, mode: str, first, second, los, squared: bool, period, observer=None) -> tuple:
    """The checked arguments of an anisotropic pair count: (a2, b2 float32 CPU tensors, los in {0,
    1, 2}, period values or None). mode 'rppi': first = rp, second = pi; 'smu': first = s, second
    = mu (always plain mu, squared by cut2_of). Under a period a line-of-sight radius (pi, s) may
    not exceed period_radius_bound of the line-of-sight axis and a perpendicular radius (rp, s)
    not that of the two other axes. los='midpoint': the third entry is the observer, a tuple of
    three finite float32 values (`observer`, None: the origin), and there is no period; an observer
    goes with no other los. ValueError otherwise; nothing on a device is read."""
    if isinstance(los, str) and los.lower() == "midpoint":
        if period is not None:
            raise ValueError(f"{what}: los='midpoint' has no period (a periodic box has no observer)")
        los = K.check_observer(what, (0.0, 0.0, 0.0) if observer is None else observer)
    else:
        if isinstance(los, str):
            los = _LOS.get(los.lower(), -1)
        if isinstance(los, bool) or not isinstance(los, int) or los not in (0, 1, 2):
            raise ValueError(f"{what}: los must be 0, 1, 2, 'x', 'y', 'z' or 'midpoint'")
        if observer is not None:
            raise ValueError(f"{what}: an observer goes with los='midpoint' only (got los={los})")
    n1, n2 = ("rp", "pi") if mode == "rppi" else ("s", "mu")
    v1, v2 = _edge_values(what, n1, first), _edge_values(what, n2, second)
    if len(v1) * len(v2) > K.PAIRS2D_MAX_CELLS:
        raise ValueError(f"{what}: {len(v1)} x {len(v2)} cells exceed {K.PAIRS2D_MAX_CELLS}")
    per = None if period is None else K.check_period(what, period)
    if per is not None:
        along = period_radius_bound((per[los],), squared)  # (an observer has no period: los is an axis)
        across = period_radius_bound(tuple(per[a] for a in range(3) if a != los), squared)
        for nm, vals, upper, axis in ((n1, v1, across, "a perpendicular axis"),
                                      (n1, v1 if mode == "smu" else (), along, "the line-of-sight axis"),
                                      (n2, v2 if mode == "rppi" else (), along, "the line-of-sight axis")):
            for r in vals:
                if float(np.float32(r)) > upper:
                    raise ValueError(f"{what}: {nm} {r} exceeds half the period of {axis} "
                                     f"({'squared ' if squared else ''}bound {upper})")
    a2 = torch.tensor([_radius_cut2(what, r, squared) for r in v1], dtype=torch.float32)
    b2 = torch.tensor([_radius_cut2(what, r, squared and mode == "rppi") for r in v2], dtype=torch.float32)
    return a2, b2, los, per


def _pairs2d(what: str, mode: str, index: LocalIndex, queries: torch.Tensor, first, second, los, squared: bool,
             period, stats: KnnStats | None, observer=None, weights: tuple | None = None) -> torch.Tensor:
    """The runner of the anisotropic pair statistics. weights: None = the counts, else (point weights,
    query weights or None) of the weighted sums."""
    a2, b2, los, per = _pairs2d_cutoffs(what, mode, first, second, los, squared, period, observer)
    midpoint = isinstance(los, tuple)  # the observer itself
    if index.qrot is not None or index.line:
        raise ValueError(f"{what}: an index built in a rotated frame or sorted by line keys is not supported")
    queries = _check_foreign(what, index, queries)
    nq, n = queries.shape[0], index.n
    pw = wq = None
    if weights is not None:
        pw = _point_weights(what, index, weights[0])
        if weights[1] is not None:
            wq = K.int64_weights(what, "query_weights", weights[1], nq, index.device)
        check_pair_sum_bound(what, pw, wq, nq)
    if nq == 0 or n == 0:
        return torch.zeros((a2.shape[0], b2.shape[0]), dtype=torch.int64, device=index.device)
    if not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        return K._pairs2d_cpu(what, index.pts[:n], queries, a2, b2, mode, los, per,
                              None if pw is None else (pw.sorted, wq), observer=midpoint)
    qsorted, qperm = prepare_queries(index, queries, locate=False)[:2]
    names = _RADIUS_STATS if per is None else _RADIUS_PERIODIC_STATS
    raw = torch.zeros(len(names), dtype=torch.int64, device=index.device) if stats is not None else None
    out = K.pair_sums_2d_gpu(index.tree(), qsorted, nq, a2, b2, mode, los, qperm, per,
                             None if pw is None else (pw.sorted, pw.prefix), wq, stats=raw)
    KERNELS_USED.add(("pair_counts_2d" if pw is None else "weighted_pair_sums_2d") + ("_observer" if midpoint else ""))
    _add_stats(stats, names, raw)
    return out


def _pairs2d_points(what: str, inner: str, mode: str, points: torch.Tensor, queries: torch.Tensor, first, second,
                    los, squared: bool, period, stats: KnnStats | None, observer=None,
                    weights: tuple | None = None) -> torch.Tensor:
    """The *_query_* / *_self_* forms: _pairs2d over an index built once from `points` (the arguments
    are checked all the same when there is nothing to index). inner: the name in the errors raised
    once there is an index (the count forms report those under their index form's name)."""
    if points.device != queries.device:
        raise ValueError(f"{what}: points on {points.device}, queries on {queries.device}")
    a2, b2 = _pairs2d_cutoffs(what, mode, first, second, los, squared, period, observer)[:2]  # (before the index)
    if points.shape[0] == 0:
        if weights is not None:
            K.int64_weights(what, "weights", weights[0], 0, points.device)
            if weights[1] is not None:
                K.int64_weights(what, "query_weights", weights[1], queries.shape[0], queries.device)
        return torch.zeros((a2.shape[0], b2.shape[0]), dtype=torch.int64, device=queries.device)
    return _pairs2d(inner, mode, build_index(points), queries, first, second, los, squared, period, stats, observer,
                    weights)


def pair_counts_rppi(index: LocalIndex, queries: torch.Tensor, rp, pi, los=2, squared: bool = False, period=None,
                     stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """int64 [Bp, Bl] on the index's device: S[i, j] = the number of pairs (query q, indexed point
    p) with perp2 < cut2_of(rp[i]) and par2 < cut2_of(pi[j]), strict and cumulative on both axes:
    the DD / DR counts of the projected two-point function along a box axis, from one walk of the
    tree and without storing a pair. shell_counts_2d(S) is the binned DD(rp, pi).

    Per pair (dx, dy, dz) are the float32 differences q - p, with `period` their minimum image
    (as radius_counts; period=(inf, inf, inf) equals the open box bit for bit). los (0, 1, 2 or
    'x', 'y', 'z') picks the line-of-sight difference dl, the other two in ascending axis order
    are da, db; par2 = dl * dl, perp2 = fmaf(db, db, da * da). A NaN component passes no test;
    a query with a NaN or infinite coordinate counts nothing. rp, pi: Python sequences or float32
    / float64 CPU tensors of 1 .. 2048 values, each >= 0, ascending, duplicates and inf allowed,
    Bp * Bl <= 65536; squared=True: the squared cutoffs themselves. Under a period every pi may
    not exceed period_radius_bound of the line-of-sight axis and every rp not that of the shorter
    finite perpendicular axis. Every argument error raises ValueError before any kernel runs,
    without a device read; an index built in a rotated frame or sorted by line keys is not
    supported. `stats` receives the radius_* counters of radius_profile. Grids of more than 2048
    cells are served in slices of whole rp rows, one walk each. Integer sums: two runs give the
    same bits. Limit as for radius_profile: whole boxes are counted without visiting their
    points, which is exact for finite indexed points.

    los='midpoint' (any case) with observer=(ox, oy, oz), three finite numbers taken as float32
    (default the origin): every pair has its own line of sight, the direction from the observer o
    to the pair's midpoint, as in survey catalogues, light cones and mocks with randoms. Open box
    only. Per pair, in float32 without contraction: l = (q - o) + (p - o) per axis (twice the
    vector observer -> midpoint), sl = fmaf(dz, lz, fmaf(dy, ly, dx * lx)), ll = dist2(lx, ly,
    lz), d2 = dist2(dx, dy, dz), par2 = (sl / ll) * sl (one correctly rounded division, one
    product), perp2 = d2 - par2, a negative perp2 becoming 0 and a NaN staying one; the cells are
    the same. Swapping q and p changes no bit, so the self forms count ordered pairs. A pair whose
    midpoint is the observer (ll == 0) counts nowhere; a point with itself has par2 = perp2 = 0;
    a NaN or infinite component or intermediate passes no test; par2 may exceed d2 by rounding
    (perp2 is then 0). The walk culls by one ball of radius² just above cut2_of(rp) + cut2_of(pi)
    of the slice and accepts no whole box (radius_box_accepts stays 0), so it evaluates more pairs
    than an axis walk. A `period`, an observer without los='midpoint' and an observer that is not
    three finite numbers raise ValueError. Not built: a periodic observer mode, sky coordinates
    (RA, Dec, z), angular w(theta), a bisector other than the midpoint."""
    return _pairs2d("pair_counts_rppi", "rppi", index, queries, rp, pi, los, squared, period, stats, observer)


def pair_query_counts_rppi(points: torch.Tensor, queries: torch.Tensor, rp, pi, los=2, squared: bool = False,
                           period=None, stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """pair_counts_rppi over an index built once from `points`, in the points' own frame."""
    return _pairs2d_points("pair_query_counts_rppi", "pair_counts_rppi", "rppi", points, queries, rp, pi, los, squared,
                           period, stats, observer)


def pair_self_counts_rppi(points: torch.Tensor, rp, pi, los=2, squared: bool = False, period=None,
                          stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """pair_query_counts_rppi with the points as their own queries: ordered pairs, (p, q) and (q,
    p) both, and every finite point with itself (perp2 = par2 = 0: in every cell with cutoffs >
    0), like pair_self_counts."""
    return pair_query_counts_rppi(points, points, rp, pi, los=los, squared=squared, period=period, stats=stats,
                                  observer=observer)


def pair_counts_smu(index: LocalIndex, queries: torch.Tensor, s, mu, los=2, squared: bool = False, period=None,
                    stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """int64 [Bs, Bm] on the index's device: S[i, j] = the number of pairs with d2 < cut2_of(s[i])
    and par2 < mu2[j] * d2 (one float32 product), mu2[j] = cut2_of(mu[j]): the cumulative counts of
    DD(s, mu) for the multipoles, mu = |dl| / s being the cosine to the line of sight. d2 is the
    canonical dist2 of the differences pair_counts_rppi describes, par2 = dl * dl. mu: always
    plain mu edges, each >= 0, ascending, inf allowed; squared=True applies to s alone. Two
    consequences of the strict product test: a pair with d2 == 0 (a point with itself, exact
    copies) counts in no column, and an edge mu = 1 excludes the pairs that lie exactly along the
    line of sight, which an edge of inf takes in. Under a period every s may exceed neither the
    bound of the line-of-sight axis nor that of a perpendicular axis. Everything else as for
    pair_counts_rppi; there is no whole-box acceptance in this mode. los='midpoint' and observer as
    for pair_counts_rppi, with its d2 and par2: since par2 may exceed d2 by rounding, an edge mu =
    1 excludes such a pair as well and an edge of inf takes it in; the cull is the ball of s."""
    return _pairs2d("pair_counts_smu", "smu", index, queries, s, mu, los, squared, period, stats, observer)


def pair_query_counts_smu(points: torch.Tensor, queries: torch.Tensor, s, mu, los=2, squared: bool = False,
                          period=None, stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """pair_counts_smu over an index built once from `points`, in the points' own frame."""
    return _pairs2d_points("pair_query_counts_smu", "pair_counts_smu", "smu", points, queries, s, mu, los, squared,
                           period, stats, observer)


def pair_self_counts_smu(points: torch.Tensor, s, mu, los=2, squared: bool = False, period=None,
                         stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """pair_query_counts_smu with the points as their own queries: ordered pairs; a point with
    itself (d2 == 0) counts nowhere."""
    return pair_query_counts_smu(points, points, s, mu, los=los, squared=squared, period=period, stats=stats,
                                 observer=observer)


def shell_counts_2d(S: torch.Tensor) -> torch.Tensor:
    """The binned counts of a cumulative [B1, B2] array of pair_counts_rppi / pair_counts_smu: its
    2-D difference, D[i, j] = S[i, j] - S[i - 1, j] - S[i, j - 1] + S[i - 1, j - 1] (terms with
    an index of -1 are 0): the pairs of cell (i, j) alone."""
    if S.dim() != 2:
        raise ValueError(f"shell_counts_2d: a [B1, B2] array is required (got {tuple(S.shape)})")
    D = S.clone()
    D[1:, :] -= S[:-1, :]
    D[:, 1:] -= D[:, :-1].clone()
    return D


# ---- weighted radius profiles: exact sums of int64 point weights within radii (radius_profile.hip)
def _max_abs(w: torch.Tensor) -> int:
    """max |w| of an int64 tensor as a Python int (one small reduction is read; |-2^63| included)."""
    if w.numel() == 0:
        return 0
    lo, hi = torch.stack(torch.aminmax(w)).tolist()
    return max(-lo, hi)


def _abs_sum(w: torch.Tensor) -> int:
    """sum |w| of an int64 tensor (fewer than 2^31 entries) as an exact Python int, whatever its
    entries: the high and the low 32 bits of the positive and of the negative entries are summed
    apart (each sum fits int64) and put together on the host. One small read."""
    if w.numel() == 0:
        return 0
    zero = torch.zeros((), dtype=torch.int64, device=w.device)
    parts = []
    for part in (torch.where(w > 0, w, zero), torch.where(w < 0, w, zero)):
        parts += [(part >> 32).sum(), (part & 0xFFFFFFFF).sum()]
    ph, pl, nh, nl = torch.stack(parts).tolist()
    return ((ph << 32) + pl) - ((nh << 32) + nl)


@dataclass
class PointWeights:
    """Per-point int64 weights prepared for one index (prepare_point_weights)."""
    index: LocalIndex
    weights: torch.Tensor                # int64 [n], rows of the indexed array
    sorted: torch.Tensor                 # the same in the index's curve order (weights[index.perm[:n]])
    prefix: torch.Tensor | None          # GPU index: int64 [n + 1] exclusive prefix sum of `sorted`
    abs_sum: int                         # A_p = sum |w|, exact


def prepare_point_weights(index: LocalIndex, weights: torch.Tensor) -> PointWeights:
    """Per-point weights (int64 [n] on the index's device, in the order of the indexed array's
    rows, negative allowed) made ready for the weighted_* functions over `index`: the weights in
    curve order and, on a GPU index, their exclusive prefix sum W (int64 [n + 1], W[0] = 0), from
    which a tree node that is accepted whole takes its weight. max|w| * n must be below 2^62
    (ValueError otherwise; one small device reduction is read): every sum of weights is then
    exact in int64. The index itself is not written. Every weighted_* function that takes an
    index accepts the result in place of the tensor, so a caller that sends queries in chunks
    prepares the weights once."""
    what = "prepare_point_weights"
    n = index.n
    w = K.int64_weights(what, "weights", weights, n, index.device)
    top = _max_abs(w)
    if top * n >= 1 << 62:
        raise ValueError(f"{what}: max|w| * n must be below 2^62 for exact int64 sums (max|w| = {top}, n = {n})")
    abs_sum = int(w.abs().sum()) if n else 0  # (cannot wrap: at most max|w| * n)
    wsorted = w[index.perm[:n].long()].contiguous()
    prefix = None
    if K.is_gpu(index.pts):
        prefix = torch.zeros(n + 1, dtype=torch.int64, device=index.device)
        torch.cumsum(wsorted, 0, out=prefix[1:])
    return PointWeights(index, w, wsorted, prefix, abs_sum)


def check_pair_sum_bound(what: str, weights: PointWeights, query_weights: torch.Tensor | None, nq: int) -> None:
    """The bound of the weighted pair sums: (sum |weights|) * (sum |query_weights|) < 2^63, with nq
    in the place of the second sum when there are no query weights (int64 [nq], on any device;
    one small read); ValueError otherwise. Every partial sum of wq * w over pairs is then exact in
    int64. The CLI applies it to a whole query file before it sends the chunks."""
    a_q = nq if query_weights is None else _abs_sum(query_weights)
    if weights.abs_sum * a_q >= 1 << 63:
        raise ValueError(f"{what}: (sum |weights|) * (sum |query_weights|) must be below 2^63 for exact int64 "
                         f"pair sums (got {weights.abs_sum} * {a_q})")


def _point_weights(what: str, index: LocalIndex, weights) -> PointWeights:
    if isinstance(weights, PointWeights):
        if weights.index is not index:
            raise ValueError(f"{what}: the point weights were prepared for another index")
        return weights
    try:
        return prepare_point_weights(index, weights)
    except ValueError as e:
        raise ValueError(str(e).replace("prepare_point_weights", what, 1)) from None


def weighted_profile(index: LocalIndex, queries: torch.Tensor, radii, weights, squared: bool = False, period=None,
                     stats: KnnStats | None = None) -> torch.Tensor:
    """int64 [nq, B], in query order: WP[q, b] = the sum of weights[p] over the points of `index`
    with dist2(q, p) < cut2_of(radii[b]), strict and cumulative, for B >= 1 ascending radii from
    one walk of the tree: radius_profile with a weight per point in the place of 1 (with unit
    weights it equals radius_profile bit for bit, and WP[q, b] is the sum of weights[idx] over
    row q of radius_neighbors at radii[b]). weights: int64 [n] on the index's device, one per
    row of the indexed array, negative allowed (data minus randoms), or the PointWeights of
    prepare_point_weights. The sums are exact, equal to the brute-force oracle bit for bit and
    independent of the index's order: max|w| * n must be below 2^62, which the host checks (one
    small device reduction is read) before any kernel runs. Float masses become such weights
    with fixed_point_weights. radii, squared, period and the limit on NaN *indexed* points as
    for radius_profile; a query with a NaN or infinite coordinate sums nothing in every column.

    Weights of another dtype, shape or device, weights prepared for another index, an overflow
    of the bound above and every argument error of radius_profile raise ValueError; an index
    built in a rotated frame or sorted by line keys is not supported. `stats` receives the
    radius_* counters of radius_profile (the two walks visit the same nodes). More radii than
    the kernel's slice width (16) are served in slices, one walk each."""
    return _profile("weighted_profile", index, queries, radii, squared, period, stats, False, (weights, None))


def weighted_pair_sums(index: LocalIndex, queries: torch.Tensor, radii, weights, query_weights=None,
                       squared: bool = False, period=None, stats: KnnStats | None = None) -> torch.Tensor:
    """int64 [B] on the index's device: WS[b] = the sum over all queries of query_weights[q] *
    weighted_profile's WP[q, b], the cumulative weighted pair sums DR(< r_b) of a two-point
    histogram (shell b holds WS[b] - WS[b - 1]), without ever allocating anything of size nq x
    B. query_weights: optional int64 [nq] on the index's device, negative allowed; None: all
    ones. Besides weighted_profile's bound, (sum |weights|) * (sum |query_weights|) (nq without
    query weights) must be below 2^63, checked on the host: every partial sum is then exact.
    Integer sums: two runs give the same bits. With unit weights this is pair_counts. Other
    arguments and errors as for weighted_profile."""
    return _profile("weighted_pair_sums", index, queries, radii, squared, period, stats, True,
                    (weights, query_weights))


def weighted_query_profile(points: torch.Tensor, queries: torch.Tensor, radii, weights: torch.Tensor,
                           squared: bool = False, period=None, stats: KnnStats | None = None) -> torch.Tensor:
    """weighted_profile over an index built once from `points` (both float32 [*, 3] on one
    device), in the points' own frame; weights: int64 [n], one per row of `points`."""
    index = _profile_index("weighted_query_profile", points, queries, radii, squared, period, (weights, None))
    if index is None:
        return torch.zeros((queries.shape[0], len(radii)), dtype=torch.int64, device=queries.device)
    return weighted_profile(index, queries, radii, weights, squared=squared, period=period, stats=stats)


def weighted_self_profile(points: torch.Tensor, radii, weights: torch.Tensor, squared: bool = False, period=None,
                          stats: KnnStats | None = None) -> torch.Tensor:
    """weighted_query_profile with the points as their own queries: every finite point adds its
    own weight (and that of its exact copies) at every radius > 0."""
    return weighted_query_profile(points, points, radii, weights, squared=squared, period=period, stats=stats)


def weighted_pair_query_sums(points: torch.Tensor, queries: torch.Tensor, radii, weights: torch.Tensor,
                             query_weights: torch.Tensor | None = None, squared: bool = False, period=None,
                             stats: KnnStats | None = None) -> torch.Tensor:
    """weighted_pair_sums over an index built once from `points`, in the points' own frame."""
    index = _profile_index("weighted_pair_query_sums", points, queries, radii, squared, period,
                           (weights, query_weights))
    if index is None:
        return torch.zeros(len(radii), dtype=torch.int64, device=queries.device)
    return weighted_pair_sums(index, queries, radii, weights, query_weights=query_weights, squared=squared,
                              period=period, stats=stats)


def weighted_pair_self_sums(points: torch.Tensor, radii, weights: torch.Tensor,
                            query_weights: torch.Tensor | None = None, squared: bool = False, period=None,
                            stats: KnnStats | None = None) -> torch.Tensor:
    """weighted_pair_query_sums with the points as their own queries and, unless query_weights is
    given, `weights` on both sides: WS[b] = sum of w[p] * w[q] over the ordered pairs with dist2
    < cut2_of(radii[b]). As pair_self_counts documents, ordered pairs are counted, (p, q) and (q,
    p) both, and every finite point with itself (w[p]^2, at every radius > 0): the unordered DD
    is the caller's (WS - WS_at_zero_distance) / 2."""
    return weighted_pair_query_sums(points, points, radii, weights,
                                    query_weights=weights if query_weights is None else query_weights,
                                    squared=squared, period=period, stats=stats)


# ---- weighted anisotropic pair sums: weights on DD(rp, pi) and DD(s, mu) (pair_counts_2d.hip)
def weighted_pair_sums_rppi(index: LocalIndex, queries: torch.Tensor, rp, pi, weights, query_weights=None, los=2,
                            squared: bool = False, period=None, stats: KnnStats | None = None,
                            observer=None) -> torch.Tensor:
    """int64 [Bp, Bl] on the index's device: WS[i, j] = the sum of query_weights[q] * weights[p]
    over the pairs (query q, indexed point p) with perp2 < cut2_of(rp[i]) and par2 < cut2_of(pi[j]),
    strict and cumulative on both axes: pair_counts_rppi with a weight per point and per query in
    the place of 1, from the same walk of the tree (with unit weights it equals pair_counts_rppi bit
    for bit, and the two walks' radius_* counters are equal). shell_counts_2d(WS) is the binned
    weighted DD(rp, pi); weights +1 on a data set and -alpha on its randoms give (D - R)(D - R).

    weights: int64 [n] on the index's device, one per row of the indexed array, negative allowed,
    or the PointWeights of prepare_point_weights; query_weights: int64 [nq] on the index's device
    or None (all ones). The sums are exact and equal the brute-force oracle bit for bit: max|w| * n
    must be below 2^62 and (sum |weights|) * (sum |query_weights|) (nq without query weights) below
    2^63, both checked on the host before any kernel runs; the device then adds and multiplies in
    wrapping 64-bit arithmetic in any order, and two runs give the same bits. Float masses become
    such weights with fixed_point_weights. rp, pi, los, squared, period, the slices of 2048 cells
    and the limit on NaN indexed points as for pair_counts_rppi; a query with a NaN or infinite
    coordinate adds nothing. Weights of another dtype, shape or device, weights prepared for
    another index, either bound exceeded and every argument error of pair_counts_rppi raise
    ValueError; an index built in a rotated frame or sorted by line keys is not supported. `stats`
    receives the radius_* counters. los='midpoint' and observer as for pair_counts_rppi."""
    return _pairs2d("weighted_pair_sums_rppi", "rppi", index, queries, rp, pi, los, squared, period, stats, observer,
                    (weights, query_weights))


def weighted_pair_query_sums_rppi(points: torch.Tensor, queries: torch.Tensor, rp, pi, weights: torch.Tensor,
                                  query_weights: torch.Tensor | None = None, los=2, squared: bool = False,
                                  period=None, stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """weighted_pair_sums_rppi over an index built once from `points`, in the points' own frame."""
    return _pairs2d_points("weighted_pair_query_sums_rppi", "weighted_pair_query_sums_rppi", "rppi", points, queries,
                           rp, pi, los, squared, period, stats, observer, (weights, query_weights))


def weighted_pair_self_sums_rppi(points: torch.Tensor, rp, pi, weights: torch.Tensor,
                                 query_weights: torch.Tensor | None = None, los=2, squared: bool = False,
                                 period=None, stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """weighted_pair_query_sums_rppi with the points as their own queries and, unless query_weights
    is given, `weights` on both sides: ordered pairs, (p, q) and (q, p) both, and every finite point
    with itself (perp2 = par2 = 0: w[p]^2 in every cell with cutoffs > 0), like
    weighted_pair_self_sums."""
    return _pairs2d_points("weighted_pair_self_sums_rppi", "weighted_pair_self_sums_rppi", "rppi", points, points, rp,
                           pi, los, squared, period, stats, observer,
                           (weights, weights if query_weights is None else query_weights))


def weighted_pair_sums_smu(index: LocalIndex, queries: torch.Tensor, s, mu, weights, query_weights=None, los=2,
                           squared: bool = False, period=None, stats: KnnStats | None = None,
                           observer=None) -> torch.Tensor:
    """int64 [Bs, Bm] on the index's device: WS[i, j] = the sum of query_weights[q] * weights[p]
    over the pairs with d2 < cut2_of(s[i]) and par2 < mu2[j] * d2: pair_counts_smu with weights, as
    weighted_pair_sums_rppi is pair_counts_rppi with weights. A pair with d2 == 0 adds to no cell;
    there is no whole-box acceptance in this mode. s, mu and everything else as for
    pair_counts_smu, weights and errors as for weighted_pair_sums_rppi."""
    return _pairs2d("weighted_pair_sums_smu", "smu", index, queries, s, mu, los, squared, period, stats, observer,
                    (weights, query_weights))


def weighted_pair_query_sums_smu(points: torch.Tensor, queries: torch.Tensor, s, mu, weights: torch.Tensor,
                                 query_weights: torch.Tensor | None = None, los=2, squared: bool = False,
                                 period=None, stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """weighted_pair_sums_smu over an index built once from `points`, in the points' own frame."""
    return _pairs2d_points("weighted_pair_query_sums_smu", "weighted_pair_query_sums_smu", "smu", points, queries,
                           s, mu, los, squared, period, stats, observer, (weights, query_weights))


def weighted_pair_self_sums_smu(points: torch.Tensor, s, mu, weights: torch.Tensor,
                                query_weights: torch.Tensor | None = None, los=2, squared: bool = False,
                                period=None, stats: KnnStats | None = None, observer=None) -> torch.Tensor:
    """weighted_pair_query_sums_smu with the points as their own queries and, unless query_weights is
    given, `weights` on both sides: ordered pairs; a point with itself (d2 == 0) adds nowhere."""
    return _pairs2d_points("weighted_pair_self_sums_smu", "weighted_pair_self_sums_smu", "smu", points, points, s,
                           mu, los, squared, period, stats, observer,
                           (weights, weights if query_weights is None else query_weights))


def fixed_point_weights(weights: torch.Tensor, n_terms: int | None = None, bits: int = 62) -> tuple:
    """(int64 tensor, s): float32 / float64 weights (masses) as exact fixed-point integers w_fix =
    rint(w * 2^-s), for the weighted_* functions; the physical value of a result is result * 2^s.
    With A = max|w| <= 2^eA (eA: its frexp exponent) and en = ceil(log2(max(n_terms or len(w),
    1))), s = eA + en - bits. The scaling is exact in float64 (a power of two) and the rounding is
    to nearest, ties to even, so the error per weight is at most 2^(s - 1), and |w_fix| <=
    2^(bits - en): any sum of up to n_terms of them (n_terms: the number of weights that can meet
    in one sum, the whole catalogue's size when it is converted in pieces) has sum |w_fix| <=
    2^bits. bits = 62 (the default) meets weighted_profile's bound.

    Pair sums multiply the two sides: weighted_pair_sums needs (sum |w|) * (sum |wq|) < 2^63, so
    the caller splits the 62 bits between the point weights and the query weights, e.g. bits=31
    for each (results then carry the quantum 2^(s_points + s_queries)); the library does not
    hide that choice. Unit query weights (query_weights=None) cost ceil(log2(nq)) bits.

    All-zero (or no) weights give zeros and s = 0. A NaN or infinite weight, a tensor that is
    not 1-D float32 / float64, n_terms < 1 or bits outside 1 .. 62 raise ValueError."""
    what = "fixed_point_weights"
    if not isinstance(weights, torch.Tensor) or weights.dtype not in (torch.float32, torch.float64) \
            or weights.dim() != 1:
        got = f"{weights.dtype} {tuple(weights.shape)}" if isinstance(weights, torch.Tensor) \
            else type(weights).__name__
        raise ValueError(f"{what}: weights must be a float32 / float64 [n] tensor (got {got})")
    if isinstance(bits, bool) or not isinstance(bits, int) or not 1 <= bits <= 62:
        raise ValueError(f"{what}: bits must be an integer in 1 .. 62 (got {bits!r})")
    if n_terms is not None and (isinstance(n_terms, bool) or not isinstance(n_terms, int) or n_terms < 1):
        raise ValueError(f"{what}: n_terms must be an integer >= 1 (got {n_terms!r})")
    w = weights.double()
    top = float(w.abs().max()) if w.numel() else 0.0
    if not math.isfinite(top):  # (a NaN propagates through max)
        raise ValueError(f"{what}: weights must be finite (no NaN, no inf)")
    if top == 0.0:
        return torch.zeros(w.shape, dtype=torch.int64, device=w.device), 0
    e_a = math.frexp(top)[1]
    e_n = (max(n_terms or w.shape[0], 1) - 1).bit_length()
    s = e_a + e_n - bits
    half = (-s) // 2  # two exact steps: 2^-s itself may lie outside float64's range
    scaled = (w * math.ldexp(1.0, half)) * math.ldexp(1.0, -s - half)
    return torch.round(scaled).to(torch.int64), s


def _no_period(what: str, period) -> None:
    if period is not None:
        raise ValueError(f"{what}: a period is not supported for per-point radii")


def point_radius_counts(index: LocalIndex, queries: torch.Tensor, point_radii, squared: bool = False,
                        stats: KnnStats | None = None, period=None) -> torch.Tensor:
    """int32 [nq], in query order: for every row of `queries` the number of points p of
    `index` whose own ball reaches it, dist2(q, p) < cut2[p] (scatter: "which points reach
    me"). point_radii: float32 [n] on the index's device in the order of the indexed array's
    rows (squared=True: squared cutoffs), or the result of prepare_point_radii for this
    index. A radius of 0 selects nothing, a point with radius inf is counted by every finite
    query; a negative or NaN entry raises ValueError before any kernel runs. The walk culls a
    node with the largest cutoff below it; there is no whole-box shortcut (it would need the
    smallest cutoff below a node), so radius_box_accepts stays 0 in `stats`. The scatter
    searches have no periodic form: a `period` raises ValueError ("not supported"); under a
    period reach_counts / reach_neighbors with query_radii=0.0 and rule="either" are this
    search."""
    _no_period("point_radius_counts", period)
    queries = _check_foreign("point_radius_counts", index, queries)
    prad = _point_radii("point_radius_counts", index, point_radii, squared)
    return _var_counts("point_radius_counts", index, queries, None, prad, stats)


def point_radius_neighbors(index: LocalIndex, queries: torch.Tensor, point_radii, squared: bool = False,
                           sort: bool = True, max_pairs: int = 1 << 28, period=None) -> tuple:
    """The CSR lists of radius_neighbors under the per-point predicate of point_radius_counts:
    row q holds every point p of `index` with dist2(q, p) < cut2[p], in the same order. No
    periodic form (see point_radius_counts): reach_neighbors with query_radii=0.0 has one."""
    _no_period("point_radius_neighbors", period)
    queries = _check_foreign("point_radius_neighbors", index, queries)
    prad = _point_radii("point_radius_neighbors", index, point_radii, squared)
    return _var_neighbors("point_radius_neighbors", index, queries, None, prad, sort, max_pairs)


def _point_query_index(what: str, points: torch.Tensor, queries: torch.Tensor) -> LocalIndex:
    if points.device != queries.device:
        raise ValueError(f"{what}: points on {points.device}, queries on {queries.device}")
    return build_index(points)


def point_radius_query_counts(points: torch.Tensor, queries: torch.Tensor, point_radii: torch.Tensor,
                              squared: bool = False, stats: KnnStats | None = None, period=None) -> torch.Tensor:
    """point_radius_counts over an index built once from `points`, in the points' own frame."""
    _no_period("point_radius_query_counts", period)
    index = _point_query_index("point_radius_query_counts", points, queries)
    return point_radius_counts(index, queries, point_radii, squared=squared, stats=stats)


def point_radius_query_neighbors(points: torch.Tensor, queries: torch.Tensor, point_radii: torch.Tensor,
                                 squared: bool = False, sort: bool = True, max_pairs: int = 1 << 28,
                                 period=None) -> tuple:
    """point_radius_neighbors over an index built once from `points`, in the points' own frame."""
    _no_period("point_radius_query_neighbors", period)
    index = _point_query_index("point_radius_query_neighbors", points, queries)
    return point_radius_neighbors(index, queries, point_radii, squared=squared, sort=sort, max_pairs=max_pairs)


def point_radius_self_neighbors(points: torch.Tensor, point_radii: torch.Tensor, squared: bool = False,
                                sort: bool = True, max_pairs: int = 1 << 28, period=None) -> tuple:
    """point_radius_query_neighbors with the points as their own queries: row i holds the
    points whose ball contains point i (with the k-th squared distances as squared radii, the
    points that have i among their k nearest, ties at the k-th distance left out)."""
    _no_period("point_radius_self_neighbors", period)
    return point_radius_query_neighbors(points, points, point_radii, squared=squared, sort=sort, max_pairs=max_pairs)


# ---- two-sided radii: a cutoff on the query and on the point at once (radius_reach.hip)
def _reach_cutoffs(what: str, index: LocalIndex, queries: torch.Tensor, query_radii, point_radii, rule: str,
                   squared: bool, period) -> tuple:
    """The checked arguments of a two-sided search: (queries, qcut2 float32 [nq], PointRadii, period
    values or None). Every ValueError of reach_counts is raised here, before any kernel runs."""
    K.reach_rule(what, rule)
    per = None if period is None else K.check_period(what, period)
    if index.qrot is not None or index.line:
        raise ValueError(f"{what}: an index built in a rotated frame or sorted by line keys is not supported")
    queries = _check_foreign(what, index, queries)
    nq, dev = queries.shape[0], index.device
    upper = None
    if per is not None and not math.isinf(period_radius_bound(per, squared)):
        upper = period_radius_bound(per, squared)
    if isinstance(query_radii, torch.Tensor):
        qcut2 = _cut2_tensor(what, "query_radii", query_radii, nq, dev, squared, upper=upper)
    elif isinstance(query_radii, (int, float)) and not isinstance(query_radii, bool):
        cut2 = _radius_cut2(what, query_radii, squared)
        if per is not None:
            check_period_radius(what, query_radii, squared, per, name="query_radii")
        qcut2 = torch.full((nq,), cut2, dtype=torch.float32, device=dev)
    else:
        raise ValueError(f"{what}: query_radii must be a float32 [{nq}] tensor or one number "
                         f"(got {type(query_radii).__name__})")
    if isinstance(point_radii, PointRadii):
        prad = _point_radii(what, index, point_radii, squared)
        if upper is not None and index.n:
            upper2 = period_radius_bound(per, True)
            if not bool((prad.cut2 <= upper2).all()):
                raise ValueError(f"{what}: every entry of point_radii must be at most half the period of every "
                                 f"finite axis (squared bound {upper2} here)")
    else:
        prad = _prepared_radii(index, _cut2_tensor(what, "point_radii", point_radii, index.n, dev, squared,
                                                   upper=upper))
    return queries, qcut2, prad, per


def _reach_counts(index: LocalIndex, queries: torch.Tensor, qcut2: torch.Tensor, prad: PointRadii, rule: str,
                  per: tuple | None, stats: KnnStats | None, _sorted: tuple | None = None) -> torch.Tensor:
    nq, n = queries.shape[0], index.n
    if nq == 0 or n == 0:
        return torch.zeros(nq, dtype=torch.int32, device=index.device)
    if not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        return K.radius_reach_count_cpu(_input_order(index), queries, qcut2, prad.cut2, rule, per)
    qsorted, qperm = _sorted if _sorted is not None else prepare_queries(index, queries, locate=False)[:2]
    names = _RADIUS_STATS if per is None else _RADIUS_PERIODIC_STATS
    raw = torch.zeros(len(names), dtype=torch.int64, device=index.device) if stats is not None else None
    tree = (index.pts, prad.nodes, index.qnodes, n, index.depth)
    counts = K.radius_reach_count_gpu(tree, qsorted, nq, qperm, qcut2, prad.cut2_sorted, rule, period=per, stats=raw)
    KERNELS_USED.add("radius_reach")
    _add_stats(stats, names, raw)
    return counts


def reach_counts(index: LocalIndex, queries: torch.Tensor, query_radii, point_radii, rule: str = "either",
                 squared: bool = False, stats: KnnStats | None = None, period=None) -> torch.Tensor:
    """int32 [nq], in query order: the two-sided radius search, a radius on the query and on the
    point at once. With cq[q] and cp[p] the squared cutoffs, p counts for q iff
        rule="either":  d2 < max(cq[q], cp[p])   (one ball reaches the other's centre)
        rule="both":    d2 < min(cq[q], cp[p])   (each ball reaches the other's centre)
    strictly, d2 the dist2 of radius_counts, under `period` its minimum image. max and min are
    taken on float32 values, so the predicate is symmetric in its bits: with smoothing lengths on
    both sides "either" is the SPH neighbour list, and with squared k-th distances as radii the
    two rules give the symmetric and the mutual k-NN graph.

    query_radii: float32 [nq] on the index's device, or one number for every query. point_radii:
    float32 [n] in the order of the indexed array's rows, or the result of prepare_point_radii
    for this index (a caller that sends queries in chunks prepares once). squared=True: both
    hold squared cutoffs. A NaN or infinite query counts nothing. Under "either" a query with
    radius 0 is still reached by points (query_radii=0.0 is point_radius_counts, and the only
    form of it under a period); under "both" a query or a point with radius 0 selects nothing.
    inf is allowed in the open box. period: as in radius_counts; every entry of both sides may
    then not exceed half the period of a finite axis. None: the open box, a walk without an
    image loop; (inf, inf, inf) gives the same result bit for bit.

    One walk serves both sides: a node is culled with max (min) of the widest live query cutoff
    and the largest point cutoff below it. Under "either" a lane counts a node whole when its own
    ball covers it (radius_box_accepts); "both" has no such shortcut. `stats` receives the
    radius_* counters and, under a period, radius_images.

    ValueError before any kernel runs: a rule other than the two; radii of a wrong type, shape
    or device; a negative or NaN entry; radii prepared for another index; under a period an
    entry above the bound, or a bad period; an index in a rotated frame or sorted by line keys."""
    queries, qcut2, prad, per = _reach_cutoffs("reach_counts", index, queries, query_radii, point_radii, rule,
                                               squared, period)
    return _reach_counts(index, queries, qcut2, prad, rule, per, stats)


def reach_neighbors(index: LocalIndex, queries: torch.Tensor, query_radii, point_radii, rule: str = "either",
                    squared: bool = False, sort: bool = True, max_pairs: int = 1 << 28, period=None) -> tuple:
    """The CSR lists of radius_neighbors under the predicate of reach_counts: row q holds every
    point p of `index` selected for q, ascending by (dist2 bits, row of the indexed array)
    (sort=False: unspecified order); dist holds the final (under a period: periodic) distances.
    More than `max_pairs` pairs raise ValueError before the lists are allocated."""
    what = "reach_neighbors"
    queries, qcut2, prad, per = _reach_cutoffs(what, index, queries, query_radii, point_radii, rule, squared, period)
    nq, n = queries.shape[0], index.n
    dev = index.device
    gpu = K.is_gpu(index.pts)
    if nq == 0 or n == 0:
        return _empty_csr(nq, dev)
    prep = prepare_queries(index, queries, locate=False)[:2] if gpu else None
    counts = _reach_counts(index, queries, qcut2, prad, rule, per, None, _sorted=prep)
    offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    total, longest = (int(v) for v in torch.stack((offsets[nq], counts.max().long())).tolist())  # the only sync
    if total > max_pairs:
        raise ValueError(f"{what}: {total} pairs within the radii exceed max_pairs = {max_pairs}; "
                         "query fewer points at a time or raise max_pairs")
    if not gpu:
        o2, idx, d2 = K.radius_reach_cpu(_input_order(index), queries, qcut2, prad.cut2, rule, per)
        return o2, idx, K.finalize_distances(d2)
    qsorted, qperm = prep
    tree = (index.pts, prad.nodes, index.qnodes, n, index.depth)
    idx, dist, err = K.radius_reach_fill_gpu(tree, index.perm, qsorted, nq, qperm, offsets, total, longest, qcut2,
                                             prad.cut2_sorted, rule, period=per, sort=sort)
    LAST_RADIUS_ERRORS[0] = int(err.item()) & 0xFFFFFFFF
    if LAST_RADIUS_ERRORS[0]:
        raise NativeError(f"{what}: {LAST_RADIUS_ERRORS[0]} rows were not filled to their count "
                          "(the count pass and the fill pass disagree: a bug)")
    return offsets, idx, dist


def reach_query_counts(points: torch.Tensor, queries: torch.Tensor, query_radii, point_radii: torch.Tensor,
                       rule: str = "either", squared: bool = False, stats: KnnStats | None = None,
                       period=None) -> torch.Tensor:
    """reach_counts over an index built once from `points`, in the points' own frame."""
    index = _point_query_index("reach_query_counts", points, queries)
    return reach_counts(index, queries, query_radii, point_radii, rule=rule, squared=squared, stats=stats,
                        period=period)


def reach_query_neighbors(points: torch.Tensor, queries: torch.Tensor, query_radii, point_radii: torch.Tensor,
                          rule: str = "either", squared: bool = False, sort: bool = True,
                          max_pairs: int = 1 << 28, period=None) -> tuple:
    """reach_neighbors over an index built once from `points`, in the points' own frame."""
    index = _point_query_index("reach_query_neighbors", points, queries)
    return reach_neighbors(index, queries, query_radii, point_radii, rule=rule, squared=squared, sort=sort,
                           max_pairs=max_pairs, period=period)


def reach_self_neighbors(points: torch.Tensor, radii: torch.Tensor, rule: str = "either", squared: bool = False,
                         sort: bool = True, max_pairs: int = 1 << 28, period=None) -> tuple:
    """reach_query_neighbors with the points as their own queries and `radii` (float32 [n]) on
    both sides: the SPH neighbour list, d2 < max(h_i, h_j)^2 ("both": min). The relation is
    symmetric: i is in row j iff j is in row i, with the same distance bits."""
    return reach_query_neighbors(points, points, radii, radii, rule=rule, squared=squared, sort=sort,
                                 max_pairs=max_pairs, period=period)


# ------------------------------------------------------------------ density clustering
# the device error word of the last cluster_labels run (tests: always 0)
LAST_CLUSTER_ERRORS = [0]
# cluster.hip `half`: a bucket's candidates above a lane's own position are left to their own
# lanes, so that each pair is united once. On by default: 1e7 uniform points, one giant
# component, 37.7 against 43.1 ms, near percolation 27.7 against 28.8 ms, no difference where
# little is linked (scripts/cluster_bench.py --no-half measures the other form)
CLUSTER_HALF = os.environ.get("LSKNN_CLUSTER_HALF", "1") != "0"
_CLUSTER_STATS = ("cluster_evals", "cluster_nodes", "cluster_buckets", "cluster_clique_accepts",
                  "cluster_cas_retries")


def _cluster_args(what: str, eps: float, min_pts: int, squared: bool) -> tuple[float, int]:
    try:
        cut2 = _radius_cut2(what, eps, squared)
    except ValueError:
        raise ValueError(f"{what}: eps must be >= 0 (got {eps})") from None
    if isinstance(min_pts, bool) or int(min_pts) != min_pts or min_pts < 1:
        raise ValueError(f"{what}: min_pts must be an integer >= 1 (got {min_pts})")
    return cut2, int(min_pts)


def _cluster_period(what: str, eps: float, cut2: float, squared: bool, period) -> tuple:
    """The checked period of a clustering: eps may not exceed half the period of a finite axis
    (r <= fl(0.5 L); squared: cut2 <= fl(h h)), which also keeps a tight node from wrapping
    inside (periodic.hip)."""
    return check_period_radius(what, eps, squared, period, name="eps")


def _cluster_periodic(index: LocalIndex, cut2: float, min_pts: int, per: tuple,
                      stats: KnnStats | None) -> tuple[torch.Tensor, torch.Tensor]:
    """cluster_labels under a period (checked arguments, n >= 1)."""
    n, dev = index.n, index.device
    if not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        return K.cluster_periodic_cpu(_input_order(index), cut2, min_pts, per)
    raw_r = torch.zeros(K.RADIUS_PERIODIC_STATS, dtype=torch.int64, device=dev) if stats is not None else None
    raw_c = torch.zeros(K.CLUSTER_STATS, dtype=torch.int64, device=dev) if stats is not None else None
    # counts in input order: the sorted points are their own queries, perm their rows
    counts = K.radius_periodic_count_gpu(index.tree(), index.pts, n, cut2, index.perm, per, stats=raw_r)
    core = counts >= min_pts
    core_sorted = core[index.perm[:n].long()].to(torch.uint8)
    labels, err = K.cluster_periodic_gpu(index.tree(), index.perm, core_sorted, cut2, per, fof=min_pts == 1,
                                         border=min_pts > 1, half=CLUSTER_HALF, stats=raw_c)
    KERNELS_USED.update(("radius_periodic", "cluster_periodic"))
    LAST_CLUSTER_ERRORS[0] = int(err.item()) & 0xFFFFFFFF  # the only host read
    if LAST_CLUSTER_ERRORS[0]:
        raise NativeError(f"cluster_labels: {LAST_CLUSTER_ERRORS[0]} parent chains did not end "
                          "(the union-find's invariant is broken: a bug)")
    _add_stats(stats, _RADIUS_PERIODIC_STATS, raw_r)
    _add_stats(stats, _CLUSTER_STATS, raw_c)
    return labels, core


def cluster_labels(index: LocalIndex, eps: float, min_pts: int = 1, squared: bool = False,
                   stats: KnnStats | None = None, period=None) -> tuple[torch.Tensor, torch.Tensor]:
    """Density clustering of the points of `index`: (labels int32 [n], core bool [n]) in the
    order of the indexed array's rows. Friends-of-friends for min_pts = 1, DBSCAN otherwise.

    Two points are linked iff dist2(p, q) < cut2_of(eps) (the strict float32 comparison of
    radius_counts; squared=True: eps is the squared cutoff itself). A point is a core point
    iff at least min_pts points, itself and exact copies included, are linked to it
    (radius_counts of the points against themselves >= min_pts). A cluster is a connected
    component of the core points under the links, and its label is the smallest row among its
    core points. A non-core point with a core point within the cutoff takes the label of the
    one smallest by (dist2 bits, row), the first core entry of its sorted radius_neighbors row;
    any other non-core point is noise, label -1. With min_pts = 1 there is no noise: a point
    without any neighbour (eps = 0, or a NaN or infinite coordinate: such a point is linked to
    nothing, itself included) is not core and forms a cluster of its own, labelled by its row.
    eps = inf puts all finite points into one cluster. The result depends on the inputs alone,
    not on the index's internal order or on the order in which the device's unions land.

    No pair is stored: the device links the components with a lock-free union-find while it
    walks the tree (cluster.hip), so memory is O(n) whatever the density. eps < 0, NaN eps or
    min_pts < 1 raise ValueError before any kernel runs; an index built in a rotated frame
    raises too. One host read (the device error word). `stats` receives cluster_evals /
    _nodes / _buckets / _clique_accepts / _cas_retries and the count pass's radius_* counters.

    period (one value or three, inf = open axis; see radius_counts): the box is periodic, two
    points are linked iff the minimum-image squared distance is below the cutoff, so a group
    that straddles a face stays one group. eps may not exceed half the period of a finite axis
    (ValueError). None: the open box, the path without this argument."""
    cut2, min_pts = _cluster_args("cluster_labels", eps, min_pts, squared)
    per = _cluster_period("cluster_labels", eps, cut2, squared, period) if period is not None else None
    if index.qrot is not None:
        raise ValueError("cluster_labels: an index built in a rotated frame cannot be clustered "
                         "(build_index(points) without a frame)")
    n, dev = index.n, index.device
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.bool, device=dev)
    if per is not None:
        return _cluster_periodic(index, cut2, min_pts, per, stats)
    if not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        return K.cluster_cpu(_input_order(index), cut2, min_pts)
    raw_r = torch.zeros(4, dtype=torch.int64, device=dev) if stats is not None else None
    raw_c = torch.zeros(K.CLUSTER_STATS, dtype=torch.int64, device=dev) if stats is not None else None
    # counts in input order: the sorted points are their own queries, perm their rows
    counts = K.radius_count_gpu(index.tree(), index.pts, n, cut2, index.perm, stats=raw_r)
    core = counts >= min_pts
    core_sorted = core[index.perm[:n].long()].to(torch.uint8)
    labels, err = K.cluster_gpu(index.tree(), index.perm, core_sorted, cut2, fof=min_pts == 1, border=min_pts > 1,
                                half=CLUSTER_HALF, stats=raw_c)
    KERNELS_USED.update(("radius", "cluster"))
    LAST_CLUSTER_ERRORS[0] = int(err.item()) & 0xFFFFFFFF  # the only host read
    if LAST_CLUSTER_ERRORS[0]:
        raise NativeError(f"cluster_labels: {LAST_CLUSTER_ERRORS[0]} parent chains did not end "
                          "(the union-find's invariant is broken: a bug)")
    _add_stats(stats, _RADIUS_STATS, raw_r)
    _add_stats(stats, _CLUSTER_STATS, raw_c)
    return labels, core


def cluster_points(points: torch.Tensor, eps: float, min_pts: int = 1, squared: bool = False,
                   stats: KnnStats | None = None, period=None) -> tuple[torch.Tensor, torch.Tensor]:
    """cluster_labels over an index built once from `points` (float32 [n, 3]), in the points'
    own frame."""
    cut2, _ = _cluster_args("cluster_points", eps, min_pts, squared)
    if period is not None:
        _cluster_period("cluster_points", eps, cut2, squared, period)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("cluster_points: points must be a float32 [n, 3] tensor")
    if points.shape[0] == 0:  # nothing to index
        return (torch.empty(0, dtype=torch.int32, device=points.device),
                torch.empty(0, dtype=torch.bool, device=points.device))
    if period is not None:
        return cluster_labels(build_index(points), eps, min_pts, squared=squared, stats=stats, period=period)
    return cluster_labels(build_index(points), eps, min_pts, squared=squared, stats=stats)


# ------------------------------------------------------------------ minimum spanning tree
# the device error word of the last mst_edges / device mst_labels run (tests: always 0)
LAST_MST_ERRORS = [0]
_MST_STATS = ("mst_evals", "mst_nodes", "mst_buckets", "mst_images", "mst_cas_retries")


def _mst_core(what: str, core_d2, n: int, device: torch.device) -> torch.Tensor | None:
    """The checked core distances: float32 [n] on `device`, every entry finite and >= 0 (one small
    device reduction is read), with -0 made +0 (the max of the contract compares bits)."""
    if core_d2 is None:
        return None
    if not isinstance(core_d2, torch.Tensor) or core_d2.dtype != torch.float32 or core_d2.dim() != 1 \
            or core_d2.shape[0] != n:
        got = f"{core_d2.dtype} {tuple(core_d2.shape)}" if isinstance(core_d2, torch.Tensor) else type(core_d2).__name__
        raise ValueError(f"{what}: core_d2 must be a float32 [{n}] tensor (got {got})")
    if core_d2.device != device:
        raise ValueError(f"{what}: core_d2 on {core_d2.device}, the index on {device}")
    if n and not bool(((core_d2 >= 0) & (core_d2 < math.inf)).all()):  # (a NaN fails the comparison too)
        raise ValueError(f"{what}: every entry of core_d2 must be finite and >= 0")
    return core_d2.contiguous() + 0.0


def _periodic_kth_d2(index: LocalIndex, per: tuple, k: int, max_pairs: int = 1 << 28) -> torch.Tensor:
    """The squared periodic k-th-neighbour distance of every point of a GPU index (n >= 1), in
    sorted positions: the flag, count and fill passes of the periodic k-NN (knn_periodic.hip) over
    the index's own points, with the k-th smallest pd2 of a flagged row taken by its bits, so no
    value passes through a square root. An unflagged point keeps its open-box value."""
    n, dev = index.n, index.device
    cfg = KnnConfig(k=int(k))
    LAST_PERIODIC_KNN_ERRORS[0] = 0
    out = torch.empty(n, dtype=torch.float32, device=dev)
    qsorted, qperm, d2 = _foreign_kth(index, index.pts[:n].contiguous(), cfg, None, out, want_d2=True)
    res = torch.empty(n, dtype=torch.float32, device=dev)
    res[qperm.long()] = d2
    if k > n or all(math.isinf(v) for v in per):  # (k > n: the cutoff under any distance)
        return res
    cutq, _, _, slices = _flagged_slices("mst_core_d2", index, per, cfg, qsorted, d2, max_pairs)
    if not slices:
        return res
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    short = torch.zeros((), dtype=torch.bool, device=dev)
    for ql, offsets, total, _ in slices:
        _, pd2 = K.pknn_fill_gpu(index.tree(), index.perm, qsorted, n, ql, cutq, per, offsets, total, err)
        # ascending by (row, bits of pd2): the k-th of every row stands at its offset + k - 1
        lens = offsets[1:] - offsets[:-1]
        row = torch.repeat_interleave(torch.arange(ql.numel(), device=dev), lens)
        key = torch.sort((row << 32) | pd2.view(torch.int32).long()).values
        have = lens >= k
        short |= (~have & (d2[ql.long()] < cfg.cut2)).any()
        take = (offsets[:-1] + (k - 1))[have]
        res[qperm[ql.long()[have]].long()] = (key[take] & 0xFFFFFFFF).int().view(torch.float32)
    LAST_PERIODIC_KNN_ERRORS[0] = (int(err.item()) & 0xFFFFFFFF) + int(short.item())
    if LAST_PERIODIC_KNN_ERRORS[0]:
        raise NativeError("mst_core_d2: a periodic row was not filled to its count or held fewer than k points "
                          "within the open-box k-th distance (a bug: that distance bounds the periodic one)")
    return res


def mst_core_d2(index: LocalIndex, k: int, period=None) -> torch.Tensor:
    """Core distances for mst_edges: float32 [n] in the order of the indexed array's rows, the
    squared distance from every point to its k-th nearest neighbour (itself counted: query's own
    value, 1 <= k <= the number of finite points), and 0 for a point with a NaN or infinite
    coordinate, which is no vertex. period (cluster_labels' values): the k-th smallest periodic
    squared distance pd2 by its bits, taken before any square root, for mst_edges(..., period=)."""
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f"mst_core_d2: k must be an integer >= 1 (got {k})")
    per = None
    if period is not None:
        per = K.check_period("mst_core_d2", period)
        if index.qrot is not None or index.line:
            raise ValueError("mst_core_d2: a period is not supported for an index built in a rotated frame or "
                             "sorted by line keys")
    n = index.n
    out = torch.zeros(n, dtype=torch.float32, device=index.device)
    if n == 0:
        return out
    if per is None:
        d2 = query(index, KnnConfig(k=int(k)), radius_hint(index.box, n, int(k)))
    elif not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        d2 = K.kth_periodic_cpu(index.pts[:n], index.pts[:n], int(k), KnnConfig(k=int(k)).cut2, per)
    else:
        d2 = _periodic_kth_d2(index, per, int(k))
    d2 = torch.where(torch.isfinite(index.pts[:n]).all(dim=1), d2[:n], torch.zeros_like(d2[:n]))
    out[index.perm[:n].long()] = d2
    return out


def _empty_mst(device: torch.device) -> tuple[torch.Tensor, torch.Tensor]:
    return (torch.empty((0, 2), dtype=torch.int32, device=device), torch.empty(0, dtype=torch.float32, device=device))


def mst_edges(index: LocalIndex, core_d2: torch.Tensor | None = None,
              stats: KnnStats | None = None, period=None) -> tuple[torch.Tensor, torch.Tensor]:
    """The Euclidean minimum spanning tree of the points of `index`: (rows int32 [m, 2], d2
    float32 [m]), the single-linkage hierarchy at every linking length at once.

    Vertices are the points with finite coordinates (a point with a NaN or infinite coordinate
    is in no edge), m = max(their number - 1, 0). The weight of the pair {a, b} is w = dist2(a,
    b), the canonical float32 squared distance every other function here compares; with core_d2
    (float32 [n] on the index's device, in the order of the indexed array's rows, every entry
    finite and >= 0, e.g. the squared k-th neighbour distances) it is the mutual-reachability
    weight max(dist2(a, b), core_d2[a], core_d2[b]), the input of HDBSCAN. Edges are ordered by
    the key (bits of w, lo, hi), lo < hi the two rows, compared lexicographically: a strict total
    order, so the tree is unique, and exact copies and lattice ties are decided by it alone.
    Each row of `rows` is (lo, hi), d2 holds w, both ascending by the key. The result depends
    on the inputs alone: not on the index's internal order, the grid, the number of rounds or
    the order in which the device's atomics land, and it equals K.mst_cpu bit for bit.

    Weights stay squared: a cut at eps compares d2 < cut2_of(eps) exactly as radius_counts does
    (mst_labels), and a square root would lose that.

    The device runs Boruvka rounds over the bucket tree (mst.hip) in O(n) memory, with one
    small host read per round (the edge counter) after one for the number of finite points; the
    components at least halve per round. A wrong core_d2 raises ValueError before any walk, as
    does an index built in a rotated frame or keyed along a line. A round beyond ceil(log2(n)),
    a final edge count other than m or a non-zero error word raise NativeError (a bug, no
    fallback). `stats` receives mst_rounds, mst_evals / _nodes / _buckets / _cas_retries and
    mst_components, the component count before every round.

    period: None, one value L or (Lx, Ly, Lz), each > 0, inf = open axis (cluster_labels' values;
    anything else raises ValueError before any kernel runs). The weight of {a, b} is then pd2(a,
    b), the float32 minimum-image squared distance of radius_counts (per axis d = q - p, h = 0.5f
    L, d > h: d - L, d < -h: d + L, then the canonical dist2; symmetric in its bits), or with
    core_d2 max(pd2, core_d2[a], core_d2[b]) (mst_core_d2(index, k, period=) gives the periodic
    core distances). Key, vertices, m and order are as above, and the result equals
    K.mst_periodic_cpu bit for bit. There is no bound on the length of an edge and no requirement
    that the coordinates lie inside one period: every pair has exactly one wrap vector in {-1, 0,
    +1}^3 by that definition. It is the physical distance of the periodic box only for
    coordinates inside one period: wrap_points brings them there. For a tree built with period=P
    and without core_d2, mst_labels(rows, d2, n, eps) equals cluster_labels(index, eps, 1,
    period=P)[0] bit for bit at every eps that cluster_labels accepts under P; above that bound
    mst_labels still works. period=(inf, inf, inf) takes the periodic path and equals the open
    result bit for bit. `stats` additionally receives mst_images, the image walks beyond image 0
    summed over waves and rounds (0 in the open box)."""
    if index.qrot is not None or index.line:
        raise ValueError("mst_edges: an index built in a rotated frame or keyed along a line cannot serve "
                         "(build_index(points) without a frame)")
    per = None if period is None else K.check_period("mst_edges", period)
    n, dev = index.n, index.device
    core = _mst_core("mst_edges", core_d2, n, dev)
    if n == 0:
        return _empty_mst(dev)
    if not K.is_gpu(index.pts):
        KERNELS_USED.add("cpu")
        return K.mst_cpu(_input_order(index), core) if per is None else \
            K.mst_periodic_cpu(_input_order(index), per, core)
    perm = index.perm[:n]
    raw = torch.zeros(K.MST_STATS, dtype=torch.int64, device=dev) if stats is not None else None
    state = K.MstState(index.tree(), index.perm, core[perm.long()].contiguous() if core is not None else None, raw,
                       period=per)
    KERNELS_USED.add("mst")
    n_finite = int(torch.isfinite(index.pts[:n]).all(dim=1).sum().item())
    want = max(n_finite - 1, 0)
    max_rounds = max(n_finite - 1, 0).bit_length()  # ceil(log2(n_finite))
    done, rounds, comps = 0, 0, []
    while done < want:
        if rounds == max_rounds:
            raise NativeError(f"mst_edges: {n_finite - done} components left after {rounds} rounds "
                              "(they must at least halve per round: a bug)")
        comps.append(n_finite - done)
        state.round()
        rounds += 1
        now = int(state.count.item()) & 0xFFFFFFFF  # the round's host read
        if now <= done:
            break
        done = now
    LAST_MST_ERRORS[0] = int(state.err.item()) & 0xFFFFFFFF
    if LAST_MST_ERRORS[0]:
        raise NativeError(f"mst_edges: error word {LAST_MST_ERRORS[0]} (an invariant of the union-find or of "
                          "the rounds is broken: a bug)")
    if done != want:
        raise NativeError(f"mst_edges: {done} edges for {n_finite} finite points (a bug)")
    if stats is not None:
        _add_stats(stats, _MST_STATS, raw)
        stats.counters["mst_rounds"] = rounds
        stats.counters["mst_components"] = comps
    rows, d2 = state.rows[:want], state.d2[:want]
    # ascending by (bits of w, lo, hi): a stable sort by hi, then one by (bits of w << 32 | lo)
    order = torch.sort(rows[:, 1], stable=True).indices
    key = (d2.view(torch.int32).long() << 32) | rows[:, 0].long()
    order = order[torch.sort(key[order], stable=True).indices]
    return rows[order].contiguous(), d2[order].contiguous()


def mst_points(points: torch.Tensor, core_d2: torch.Tensor | None = None,
               stats: KnnStats | None = None, period=None) -> tuple[torch.Tensor, torch.Tensor]:
    """mst_edges over an index built once from `points` (float32 [n, 3]), in the points' own
    frame. period: see mst_edges."""
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("mst_points: points must be a float32 [n, 3] tensor")
    if period is not None:  # (before an index is built)
        K.check_period("mst_points", period)
    if points.shape[0] == 0:  # nothing to index
        _mst_core("mst_points", core_d2, 0, points.device)
        return _empty_mst(points.device)
    return mst_edges(build_index(points), core_d2, stats=stats, period=period)


def mst_labels(rows: torch.Tensor, d2: torch.Tensor, n: int, eps: float, squared: bool = False) -> torch.Tensor:
    """The single-linkage clusters at one linking length from the tree of mst_edges: labels
    int32 [n], the connected components of the edges with d2 < cut2_of(eps) (the strict float32
    comparison of radius_counts; squared=True: eps is the squared cutoff itself), each labelled
    by its smallest row; a row in no such edge is labelled by itself. For a tree built without
    core_d2 this equals cluster_labels(index, eps, min_pts=1)[0] bit for bit: two points are in
    one friends-of-friends group iff a path of pairs below the cutoff joins them, iff the path
    between them in the minimum spanning tree stays below it. The weights are squared distances
    and must stay so: the cut compares them with the squared cutoff. Device tensors run the edge
    hook of mst.hip and the label passes of cluster.hip (one host read, the error word), CPU
    tensors the host runtime."""
    try:
        cut2 = _radius_cut2("mst_labels", eps, squared)
    except ValueError:
        raise ValueError(f"mst_labels: eps must be >= 0 (got {eps})") from None
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"mst_labels: n must be an integer >= 0 (got {n})")
    n = int(n)
    if not isinstance(rows, torch.Tensor) or not isinstance(d2, torch.Tensor) or rows.dtype != torch.int32 \
            or d2.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 2 or d2.dim() != 1 \
            or rows.shape[0] != d2.shape[0]:
        raise ValueError("mst_labels: rows must be an int32 [m, 2] tensor and d2 a float32 [m] tensor")
    if rows.device != d2.device:
        raise ValueError(f"mst_labels: rows on {rows.device}, d2 on {d2.device}")
    if d2.shape[0] > max(n - 1, 0):
        raise ValueError(f"mst_labels: {d2.shape[0]} edges are no forest over {n} rows")
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=d2.device)
    if not K.is_gpu(d2):
        return K.mst_labels_cpu(rows, d2, n, cut2)
    labels, err = K.mst_labels_gpu(rows, d2, n, cut2)
    KERNELS_USED.update(("mst", "cluster"))
    LAST_MST_ERRORS[0] = int(err.item()) & 0xFFFFFFFF  # the only host read
    if LAST_MST_ERRORS[0]:
        raise NativeError(f"mst_labels: error word {LAST_MST_ERRORS[0]} (an edge names a row outside [0, {n}), or "
                          "the union-find's invariant is broken)")
    return labels


def compact_labels(labels: torch.Tensor) -> tuple[torch.Tensor, int]:
    """(dense int32 labels, number of clusters): the clusters of cluster_labels numbered 0, 1,
    ... by ascending label (the smallest row of their core points); -1 stays -1."""
    noise = labels < 0
    uniq, inv = torch.unique(labels[~noise], sorted=True, return_inverse=True)
    dense = torch.full_like(labels, -1, dtype=torch.int32)
    dense[~noise] = inv.to(torch.int32)
    return dense, int(uniq.numel())
