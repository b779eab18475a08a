"""Plain references and fixtures for the halo-filter, partition and result-return kernels
(test_halo_cpu.py, test_gpu_halo.py).

The box tests of the kernels use the canonical float32 formula of common.h (box_dist2 /
dist2 with fmaxf, which ignores a NaN operand). The reference here is a float64 bracket:
for every (point or box, leaf) pair the squared gap is computed in float64 from the
float32 inputs (torch.fmax: the same NaN rule), and two sets are formed with strict `<`:

    must = gap2 < r2 * (1 - 2^-20)        may = gap2 < r2 * (1 + 2^-19)

A kernel's output is right iff must <= got <= may after the kernel's own reduction (over
leaves, over points). The margins are derived: the float32 formula has at most 5
roundings of 2^-24 each, and the CPU form of boundary_groups shrinks its gap by 2^-20,
which the 2^-19 of `may` covers. `bracket_share` is the share of pairs in may \\ must:
the tests assert it stays at or below 0.1 %, so the bracket cannot hide a failure.
"""
import functools
import math

import numpy as np
import torch

from datasets import GENERATORS
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

INF = math.inf
NAN = math.nan
SUBNORMAL = 2.0 ** -149          # the smallest positive float32
MUST = 1.0 - 2.0 ** -20
MAY = 1.0 + 2.0 ** -19
MAX_SHARE = 1e-3                 # may \ must pairs / may pairs
SENTINEL = 0x5A5A5A5A            # int32 pattern of untouched output words
GENS = ("uniform", "clustered", "duplicates", "planar")
SHARD_SIZES = (3100, 3600, 4000)  # 49 / 57 / 63 buckets: depth 6, no power of two


def bits(t: torch.Tensor) -> torch.Tensor:
    """The int32 bit patterns of a float32 / int32 tensor (on the CPU)."""
    return t.detach().cpu().contiguous().view(torch.int32)


# --------------------------------------------------------------------------- gaps, bracket
def point_gap2(pts: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
    """float64 [n, L]: squared gap of every point to every box (8-float rows)."""
    p = pts.double()[:, None, :]
    lo, hi = boxes[:, 0:3].double()[None], boxes[:, 4:7].double()[None]
    g = torch.fmax(torch.fmax(lo - p, p - hi), torch.zeros((), dtype=torch.float64))
    return (g * g).sum(-1)


def box_gap2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """float64 [G, L]: squared gap between every box of a and every box of b."""
    alo, ahi = a[:, None, 0:3].double(), a[:, None, 4:7].double()
    blo, bhi = b[None, :, 0:3].double(), b[None, :, 4:7].double()
    g = torch.fmax(torch.zeros((), dtype=torch.float64), torch.fmax(alo - bhi, blo - ahi))
    return (g * g).sum(-1)


def bracket(gap2: torch.Tensor, r2: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(must, may) bool of the shape of gap2; r2 (float32 values) broadcasts against it."""
    r = r2.double()
    return gap2 < r * MUST, gap2 < r * MAY


class Share:
    """Counts the pairs of may and of may \\ must over the calls of one test."""

    def __init__(self):
        self.may = 0
        self.slack = 0

    def add(self, must: torch.Tensor, may: torch.Tensor) -> None:
        assert not bool((must & ~may).any())
        self.may += int(may.sum())
        self.slack += int((may & ~must).sum())

    def check(self, what: str = "") -> None:
        print(f"bracket {what}: may pairs {self.may}, may \\ must {self.slack}")
        assert self.slack <= MAX_SHARE * self.may, (what, self.slack, self.may)


# --------------------------------------------------------------------------- tree radii
def ref_tree_radii(nodes: torch.Tensor, n: int, d2: torch.Tensor) -> torch.Tensor:
    """A copy of the CPU node array with the expected lo.w column of tree_set_radii: leaf =
    max over the bucket's valid entries with NaN counted as +inf, entries at or past n as
    0; every inner node (down to node 1) = max over the leaves below it."""
    slots = nodes.shape[0] // 2
    depth = slots.bit_length() - 1
    r = torch.zeros(slots * 64, dtype=torch.float32)
    d = d2[:n].detach().cpu().float()
    r[:n] = torch.where(torch.isnan(d), torch.full_like(d, INF), d)
    leaf = r.view(slots, 64).max(dim=1).values
    out = nodes.clone()
    for level in range(depth + 1):
        out[(1 << level):(2 << level), 3] = leaf.view(1 << level, -1).max(dim=1).values
    return out


def radii_case(n: int, mode: str, seed: int = 0) -> torch.Tensor:
    """d2 [n]: random positive with 0, +inf and a subnormal injected, an all-NaN bucket
    and a single NaN in the last valid lane of the last bucket. With fewer than three
    buckets the two NaN patterns cannot coexist: `mode` ("all" / "last") picks one."""
    g = torch.Generator().manual_seed(1000 + seed + n)
    d2 = torch.rand(n, generator=g) * 0.01 + 1e-6
    nb = (n + 63) // 64
    if n >= 4:
        d2[0], d2[n // 2] = 0.0, SUBNORMAL
    if n >= 4 and (nb >= 3 or mode == "all"):
        d2[n // 3] = INF  # (never in the bucket of the single NaN: it would hide a lost NaN)
    if nb >= 3:
        d2[64:128] = NAN
        d2[n - 1] = NAN
    elif mode == "all":
        d2[(nb - 1) * 64:] = NAN
    else:
        d2[n - 1] = NAN
    return d2


def sentinel_nodes(n: int, seed: int = 0) -> torch.Tensor:
    """[2^(depth+1), 8] float32 of random finite bit patterns (no NaN: bitwise compares of
    every untouched column stay meaningful through a device copy)."""
    rows = 2 << K.tree_depth(n)
    g = torch.Generator().manual_seed(77 + seed + n)
    return (torch.rand((rows, 8), generator=g) * 200.0 - 100.0).float()


# --------------------------------------------------------------------------- shards
class Shards:
    """P rank shards of one data set: per rank the curve-sorted points, the tree built on
    `dev` (copied to the CPU, node 0 zeroed) with the k = 8 radii and with synthetic
    radii, all as CPU tensors."""

    def __init__(self, gen: str, dev: torch.device, seed: int):
        p = GENERATORS[gen](sum(SHARD_SIZES), seed=seed)
        p = p[torch.sort(p[:, 0], stable=True).indices]  # slabs along x: real halos
        self.gen, self.pts, self.nodes_k8, self.nodes_syn, self.n = gen, [], [], [], []
        g = torch.Generator().manual_seed(seed + 5)
        spacing2 = (1.0 / p.shape[0]) ** (2.0 / 3.0)
        s = 0
        for j, nj in enumerate(SHARD_SIZES):
            idx = E.build_index(p[s:s + nj].to(dev))
            s += nj
            assert idx.depth == 6
            pts = idx.pts[:nj].cpu()
            nodes = idx.nodes.cpu().clone()
            nodes[0] = 0.0
            nodes[:, 3] = 0.0
            d2 = K.kth_cpu(pts, pts, 8, INF)
            # synthetic: log-uniform around the mean spacing; a zero bucket, a subnormal
            # bucket, and +inf in one bucket of the last rank only (an infinite radius
            # sends every finite point: the other ranks keep a selective filter)
            syn = spacing2 * 10.0 ** (torch.rand(nj, generator=g) * 2.0 - 1.0)
            syn[0:64] = 0.0
            syn[64:128] = SUBNORMAL
            if j == len(SHARD_SIZES) - 1:
                syn[5 * 64 + 7] = INF
            self.pts.append(pts)
            self.n.append(nj)
            self.nodes_k8.append(ref_tree_radii(nodes, nj, d2))
            self.nodes_syn.append(ref_tree_radii(nodes, nj, syn))

    def nodes(self, variant: str) -> list:
        return self.nodes_k8 if variant == "k8" else self.nodes_syn


@functools.lru_cache(maxsize=None)
def shards(gen: str, dev_str: str, seed: int = 11) -> Shards:
    return Shards(gen, torch.device(dev_str), seed)


@functools.lru_cache(maxsize=None)
def own_points(gen: str, n: int = 9477, seed: int = 23) -> torch.Tensor:
    """Points tested against the published trees: over the whole cube, so that every rank's
    slab has points inside, near and far."""
    return GENERATORS[gen](n, seed=seed).contiguous()


# --------------------------------------------------------------------------- publication
def publish(nodes: list, depths: list, levels: int):
    """The published buffer as pipelines._publish lays it out: per rank `rows = 2 << levels`
    rows, the first 2 << depth of them the rank's tree, unused rows lo = +inf, hi = -inf,
    r2 = 0, the depth in row 0's last column. Returns ([P, rows, 8], float offsets, depths)."""
    rows = 2 << levels
    pub = torch.zeros((len(nodes), rows, 8), dtype=torch.float32)
    pub[:, :, 0:3] = INF
    pub[:, :, 4:7] = -INF
    for j, (nd, d) in enumerate(zip(nodes, depths)):
        take = 2 << d
        assert take <= rows and take <= nd.shape[0]
        pub[j, :take] = nd[:take]
        pub[j, 0, 7] = float(d)
    return pub, [j * rows * 8 for j in range(len(nodes))], list(depths)


def one_leaf(lo, hi, r2) -> torch.Tensor:
    """A depth-0 tree: node 0 unused, node 1 the box with its squared radius."""
    nd = torch.zeros((2, 8), dtype=torch.float32)
    nd[1, 0:3] = torch.tensor(lo, dtype=torch.float32)
    nd[1, 4:7] = torch.tensor(hi, dtype=torch.float32)
    nd[1, 3] = r2
    return nd


def pub_leaves(pub: torch.Tensor, depths: list, j: int) -> torch.Tensor:
    return pub[j, (1 << depths[j]):(2 << depths[j])]


def mask_bracket(pts: torch.Tensor, pub: torch.Tensor, depths: list, self_rank: int, share: Share):
    """(must, may) int64 masks of halo_mask: bit j iff some published leaf of rank j != self
    has the point strictly inside its radius."""
    must = torch.zeros(pts.shape[0], dtype=torch.int64)
    may = torch.zeros(pts.shape[0], dtype=torch.int64)
    for j in range(pub.shape[0]):
        if j == self_rank:
            continue
        lv = pub_leaves(pub, depths, j)
        mu, ma = bracket(point_gap2(pts, lv), lv[None, :, 3])
        share.add(mu, ma)
        must |= mu.any(1).to(torch.int64) << j
        may |= ma.any(1).to(torch.int64) << j
    return must, may


def assert_mask_in_bracket(got: torch.Tensor, must: torch.Tensor, may: torch.Tensor) -> None:
    got = got.cpu()
    assert bool(((must & ~got) == 0).all()), "a must pair is missing (dropped candidate)"
    assert bool(((got & ~may) == 0).all()), "a bit outside may is set (over-wide filter)"


def hierarchy_mask(pts: torch.Tensor, pub: torch.Tensor, depths: list, self_rank: int) -> torch.Tensor:
    """The must mask by a walk of the hierarchy (a node is entered only when the point is
    inside its own radius): equal to the leaf-only reduction when every parent box encloses
    its children and carries their maximum radius."""
    out = torch.zeros(pts.shape[0], dtype=torch.int64)
    for j in range(pub.shape[0]):
        if j == self_rank:
            continue
        alive = torch.ones((pts.shape[0], 1), dtype=torch.bool)
        for level in range(depths[j] + 1):
            nd = pub[j, (1 << level):(2 << level)]
            if level:
                alive = alive.repeat_interleave(2, dim=1)
            alive = alive & bracket(point_gap2(pts, nd), nd[None, :, 3])[0]
        out |= alive.any(1).to(torch.int64) << j
    return out


# the strictness rows of halo_mask / flag_groups_inverse against a one-leaf tree with the box
# [0,1]^3: (point, inside r2 = 0.25, inside r2 = 0, inside r2 = +inf)
def hand_rows():
    below = float(np.nextafter(np.float32(1.5), np.float32(0.0)))
    above = float(np.nextafter(np.float32(-0.5), np.float32(0.0)))
    rows = [
        ((1.5, 0.5, 0.5), 0, 0, 1),        # gap2 == r2: strict <, not sent
        ((below, 0.5, 0.5), 1, 0, 1),      # one ulp closer: sent
        ((0.5, 0.5, 0.5), 1, 0, 1),        # inside the box: gap 0, r2 = 0 still sends nothing
        ((INF, 0.5, 0.5), 0, 0, 0),        # inf < inf is false
        # a NaN coordinate vanishes in fmaxf: that axis' gap is 0 (the canonical formula's
        # behaviour, pinned to the CPU twin; not a bug to fix in the filter)
        ((NAN, 0.5, 0.5), 1, 0, 1),
        ((NAN, 5.0, 0.5), 0, 0, 1),
        ((-0.5, 0.5, 0.5), 0, 0, 1),
        ((0.5, above, 0.5), 1, 0, 1),
        ((0.5, 0.5, -INF), 0, 0, 0),
    ]
    pts = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    return pts, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]


# --------------------------------------------------------------------------- masks, flags
def random_masks(n: int, nranks: int, seed: int, kind: str = "random") -> torch.Tensor:
    """int64 [n] with random bits below nranks; "waves": whole 64-point waves zeroed;
    "zero": all zero."""
    g = torch.Generator().manual_seed(seed + 64 * n + nranks)
    lo = torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64)
    hi = torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64)
    m = (hi << 32) | lo
    if nranks < 64:
        m &= (1 << nranks) - 1
    if kind == "zero":
        m.zero_()
    elif kind == "waves":
        w = torch.arange(n) // 64
        m[(w % 3) == 1] = 0
    return m


def bit_counts(mask: torch.Tensor, nranks: int) -> torch.Tensor:
    return torch.stack([((mask >> j) & 1).sum() for j in range(nranks)]).to(torch.int32)


def sorted_rows(rows: torch.Tensor) -> np.ndarray:
    """[m, 3] float rows sorted by their int32 bit patterns (a multiset compare)."""
    b = bits(rows).numpy().reshape(-1, 3)
    return b[np.lexsort((b[:, 2], b[:, 1], b[:, 0]))]


def flag_case(n: int, density: float, seed: int = 0) -> torch.Tensor:
    """int32 [n] flags: `density` of them set, to 1, 7 or 0x80000000."""
    g = torch.Generator().manual_seed(seed + n)
    on = torch.rand(n, generator=g) < density if 0.0 < density < 1.0 else torch.full((n,), density >= 1.0)
    val = torch.tensor([1, 7, -(1 << 31)], dtype=torch.int32)[torch.randint(0, 3, (n,), generator=g)]
    return torch.where(on, val, torch.zeros(n, dtype=torch.int32))


# --------------------------------------------------------------------------- partition
SHIFT = 14  # 30-bit keys, 16-bit bins (pipelines.SPLIT_BITS)


def key_case(n: int, splitters: list, seed: int = 0) -> torch.Tensor:
    """int32 [n] 30-bit keys: random, with every fifth key's bin set to a splitter (or to
    bin 0 / the largest bin) so that bins equal to a splitter occur."""
    g = torch.Generator().manual_seed(seed + n)
    keys = torch.randint(0, 1 << 30, (n,), generator=g, dtype=torch.int64)
    special = torch.tensor(list(splitters) + [0, 65535], dtype=torch.int64)
    pick = special[torch.randint(0, special.shape[0], (n,), generator=g)]
    every = (torch.arange(n) % 5) == 0
    keys = torch.where(every, (pick << SHIFT) | (keys & ((1 << SHIFT) - 1)), keys)
    return keys.to(torch.int32)


def ref_dest(keys: torch.Tensor, splitters: list) -> torch.Tensor:
    split = torch.tensor(splitters, dtype=torch.int64)
    return torch.searchsorted(split, keys.to(torch.int64) >> SHIFT, right=True).to(torch.int32)


SPLITTER_CASES = {
    "none": [],
    "plain": [9000, 30000, 51000],
    "duplicate": [20000, 20000, 40000],   # rank 2 is empty
    "ends": [0, 65535],                   # rank 0 is empty; the largest bin is a rank of its own
}


# --------------------------------------------------------------------------- finalize
def d2_case(n: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed + n)
    d2 = torch.rand(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 20.0 - 10.0)
    special = [0.0, INF, NAN, SUBNORMAL, 2.0 ** -126, 3.0e38]
    for i, v in enumerate(special[:n]):
        d2[(i * 37) % n] = v
    return d2.float()


def ref_final(d2: torch.Tensor) -> torch.Tensor:
    """sqrt on the CPU, correctly rounded: the float64 square root rounded once to float32
    (53 >= 2 * 24 + 2 bits: the double rounding is exact). +inf stays, NaN stays NaN."""
    return torch.sqrt(d2.cpu().double()).float()


def assert_same_floats(got: torch.Tensor, ref: torch.Tensor) -> None:
    """Bitwise equal, any NaN matching any NaN."""
    got, ref = got.cpu(), ref.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(bits(got)[~nan], bits(ref)[~nan])
