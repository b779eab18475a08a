"""The CPU twins of the halo-filter, partition and result-return kernels against the plain
references of halo_ref.py: box tests within the float64 bracket (must <= got <= may),
everything else exact. Runs anywhere; test_gpu_halo.py holds the same checks for the
kernels and pins them to these twins."""
import math

import pytest
import torch

import halo_ref as R
from datasets import clustered, uniform
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.parallel import pipelines as PL
from mpi_cuda_largescaleknn_amd.parallel.comm import run_loopback

CPU = "cpu"
DEPTH_MIXES = [(6, 6, 6), (0, 3, 6), (3, 6, 0), (0, 0, 0)]


# --------------------------------------------------------------------------- 1. tree_set_radii
@pytest.mark.parametrize("mode", ["all", "last"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 4097, 10_000])
def test_tree_set_radii_cpu(n, mode):
    d2 = R.radii_case(n, mode)
    nodes = R.sentinel_nodes(n)
    ref = R.ref_tree_radii(nodes, n, d2)
    got = K.tree_set_radii(nodes.clone(), n, d2)
    assert not bool(torch.isnan(got[1:, 3]).any())
    assert torch.equal(R.bits(got), R.bits(ref))          # radii, untouched columns, node 0
    slots, nb = nodes.shape[0] // 2, (n + 63) // 64
    assert float(got[slots + nb - 1, 3]) == math.inf      # the NaN of the last valid lane
    assert float(got[1, 3]) == math.inf
    assert bool((got[slots + nb:, 3] == 0).all())         # leaf slots past the last bucket
    assert torch.equal(R.bits(got[0]), R.bits(nodes[0]))  # node 0: the radius hint
    if nb >= 3:
        assert float(got[slots + 1, 3]) == math.inf       # the all-NaN bucket
        assert float(got[slots + 2, 3]) == float(d2[128:192].max())


def test_tree_radii_levelup_ignores_nan():
    """The inner levels take fmaxf of their children (levelup_kernel): a NaN leaf radius
    that reaches them some other way must not replace a number."""
    nodes = torch.zeros((8, 8))
    nodes[4:, 3] = torch.tensor([1.0, math.nan, math.nan, 3.0])
    K._levelup_radii(nodes, 2)
    assert nodes[1:4, 3].tolist() == [3.0, 1.0, 3.0]


# --------------------------------------------------------------------------- 2. halo_mask
def cpu_mask(pts, pub, offs, depths, self_rank):
    return K.halo_mask(pts, pub.reshape(-1), offs, depths, self_rank)


@pytest.mark.parametrize("variant", ["k8", "syn"])
@pytest.mark.parametrize("gen", R.GENS)
def test_halo_mask_cpu_bracket(gen, variant):
    S = R.shards(gen, CPU)
    pts = R.own_points(gen)
    share = R.Share()
    for depths in DEPTH_MIXES:
        pub, offs, depths = R.publish(S.nodes(variant), depths, 6)
        must, may = R.mask_bracket(pts, pub, depths, 1, share)
        got = cpu_mask(pts, pub, offs, torch.tensor(depths, dtype=torch.int32), 1)
        R.assert_mask_in_bracket(got, must, may)
        assert bool((got & ~0b101 == 0).all())  # never the self bit, never a bit >= nranks
        # the reduction over published leaves equals a walk of the hierarchy
        assert torch.equal(R.hierarchy_mask(pts, pub, depths, 1), must)
    share.check(f"halo_mask {gen} {variant}")
    if variant == "syn" or gen != "duplicates":
        assert share.may > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 9_477])
def test_halo_mask_cpu_sizes(n):
    S = R.shards("uniform", CPU)
    pts = R.own_points("uniform")[:n].contiguous()
    pub, offs, depths = R.publish(S.nodes("k8"), (0, 3, 6), 6)
    share = R.Share()
    must, may = R.mask_bracket(pts, pub, depths, 1, share)
    R.assert_mask_in_bracket(cpu_mask(pts, pub, offs, depths, 1), must, may)
    share.check(f"halo_mask sizes n={n}")


@pytest.mark.parametrize("r2_other", [0.0, math.inf])
def test_halo_mask_cpu_hand_rows(r2_other):
    pts, in_quarter, in_zero, in_inf = R.hand_rows()
    box = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    pub, offs, depths = R.publish([R.one_leaf(*box, 0.25), R.one_leaf(*box, math.inf),
                                   R.one_leaf(*box, r2_other)], (0, 0, 0), 0)
    other = in_zero if r2_other == 0.0 else in_inf
    expect = torch.tensor([a | (b << 2) for a, b in zip(in_quarter, other)], dtype=torch.int64)
    assert torch.equal(cpu_mask(pts, pub, offs, depths, 1), expect)


def test_halo_mask_cpu_padded_rows_never_hit():
    """A depth-1 tree whose second leaf is an unused row (lo = +inf, hi = -inf): no point
    reaches it, whatever radius the row carries."""
    pts, in_quarter, _, _ = R.hand_rows()
    finite = ~torch.isnan(pts).any(1)
    for pad_r2 in (0.0, math.inf):
        nd = torch.zeros((4, 8))
        nd[:, 0:3], nd[:, 4:7] = math.inf, -math.inf
        nd[1] = R.one_leaf((0, 0, 0), (1, 1, 1), max(0.25, pad_r2))[1]
        nd[2] = R.one_leaf((0, 0, 0), (1, 1, 1), 0.25)[1]
        nd[3, 3] = pad_r2
        pub, offs, depths = R.publish([nd, nd], (1, 1), 1)
        got = cpu_mask(pts[finite].contiguous(), pub, offs, depths, 1)
        assert got.tolist() == [b for b, f in zip(in_quarter, finite.tolist()) if f]


def sixty_four_ranks():
    """64 one-leaf trees, rank j's box [j, j+1] x [0,1]^2 with r2 = 0.01, and points over all
    of them."""
    nodes = [R.one_leaf((j, 0, 0), (j + 1, 1, 1), 0.01) for j in range(64)]
    pts = uniform(1000, seed=64) * torch.tensor([64.0, 1.0, 1.0])
    return R.publish(nodes, [0] * 64, 0), pts.contiguous()


def test_halo_mask_cpu_64_ranks():
    (pub, offs, depths), pts = sixty_four_ranks()
    share = R.Share()
    must, may = R.mask_bracket(pts, pub, depths, 0, share)
    got = cpu_mask(pts, pub, offs, depths, 0)
    R.assert_mask_in_bracket(got, must, may)
    share.check("halo_mask 64 ranks")
    assert bool((got < 0).any()) and bool((got & 1 == 0).all())  # bit 63 works, no self bit


def test_halo_mask_cpu_65_ranks_raises():
    nodes = [R.one_leaf((j, 0, 0), (j + 1, 1, 1), 0.01) for j in range(65)]
    pub, offs, depths = R.publish(nodes, [0] * 65, 0)
    with pytest.raises(ValueError):
        cpu_mask(uniform(10), pub, offs, depths, 0)


# --------------------------------------------------------------------------- 4. compact_flags
@pytest.mark.parametrize("density", [0.0, 1.0 / 64.0, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 10_000])
def test_compact_flags_cpu(n, density):
    flags = R.flag_case(n, density)
    lst, cnt = K.compact_flags(flags)
    expect = torch.nonzero(flags).view(-1).to(torch.int32)
    assert int(cnt) == expect.shape[0]
    assert torch.equal(torch.sort(lst[:int(cnt)]).values, expect)


# --------------------------------------------------------------------------- 6. boundary_groups
def boundary_bracket(local, depth, ngroups, pub, depths, self_rank, share):
    leaves = local[(1 << depth):(1 << depth) + ngroups]
    must = torch.zeros(ngroups, dtype=torch.bool)
    may = torch.zeros(ngroups, dtype=torch.bool)
    for j in range(pub.shape[0]):
        if j == self_rank:
            continue
        mu, ma = R.bracket(R.box_gap2(leaves, R.pub_leaves(pub, depths, j)), leaves[:, None, 3])
        share.add(mu, ma)
        must |= mu.any(1)
        may |= ma.any(1)
    return must, may


def local_tree(dev, variant, gen="uniform"):
    """(CPU copy of a 300-bucket tree, its depth 9) with a-priori k = 8 radius bounds, or with
    synthetic leaf radii that include 0 and +inf."""
    n = 300 * 64 - 50
    idx = E.build_index(R.own_points(gen, n, seed=31).to(dev))
    nodes = K.tree_set_radii_ub(idx.nodes.clone(), idx.pts, n, 8).cpu()
    if variant == "syn":
        g = torch.Generator().manual_seed(3)
        nodes[512:, 3] = 1e-3 * 10.0 ** (torch.rand(512, generator=g) * 2.0 - 1.0)
        nodes[512 + 3::17, 3] = 0.0
        nodes[512 + 5::41, 3] = math.inf
    nodes[0] = 0.0
    return nodes, idx.depth


@pytest.mark.parametrize("variant", ["ub", "syn"])
@pytest.mark.parametrize("ngroups", [1, 63, 65, 300])
def test_boundary_groups_cpu_bracket(ngroups, variant):
    local, depth = local_tree(torch.device(CPU), variant)
    assert depth == 9
    share = R.Share()
    for gen in ("uniform", "planar"):
        S = R.shards(gen, CPU)
        pub, offs, depths = R.publish(S.nodes("k8"), (0, 3, 6), 6)
        must, may = boundary_bracket(local, depth, ngroups, pub, depths, 1, share)
        got = K.boundary_groups(local, depth, ngroups, pub.reshape(-1), offs, depths, 1).bool()
        assert bool((must <= got).all()) and bool((got <= may).all())
    share.check(f"boundary_groups {variant} {ngroups}")


def test_boundary_groups_cpu_depth0_local_tree():
    S = R.shards("uniform", CPU)
    share = R.Share()
    for r2 in (0.0, 1e-3, 0.3, math.inf):
        local = R.one_leaf((0.2, 0.2, 0.2), (0.25, 0.3, 0.3), r2)
        pub, offs, depths = R.publish(S.nodes("k8"), (3, 6, 0), 6)
        must, may = boundary_bracket(local, 0, 1, pub, depths, 1, share)
        got = K.boundary_groups(local, 0, 1, pub.reshape(-1), offs, depths, 1).bool()
        assert bool((must <= got).all()) and bool((got <= may).all())
        assert bool(got[0]) == (r2 > 0.0)  # the box lies inside rank 0's slab: gap 0
    share.check("boundary_groups depth 0")


# --------------------------------------------------------------------------- 7. partition
@pytest.mark.parametrize("case", list(R.SPLITTER_CASES))
@pytest.mark.parametrize("n", [1, 1_023, 1_025, 300_001])
def test_dest_and_perm_cpu(n, case):
    splitters = R.SPLITTER_CASES[case]
    keys = R.key_case(n, splitters)
    size = len(splitters) + 1
    dest = R.ref_dest(keys, splitters).to(torch.int64)
    perm, counts = PL._dest_and_perm(keys, splitters, size)
    assert torch.equal(perm.to(torch.int64), torch.sort(dest, stable=True).indices)
    assert torch.equal(counts.to(torch.int64), torch.bincount(dest, minlength=size))


# --------------------------------------------------------------------------- 8. scatter1, finalize
@pytest.mark.parametrize("n", [1, 257, 100_001])
def test_scatter1_finalize_cpu(n):
    d2 = R.d2_case(n)
    R.assert_same_floats(K.finalize_distances(d2), R.ref_final(d2))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    for fin in (False, True):
        out = torch.full((n + 3,), -7.0)
        K.scatter1(d2, perm.to(torch.int32), out, fin)
        ref = torch.full((n + 3,), -7.0)
        ref[perm] = R.ref_final(d2) if fin else d2
        R.assert_same_floats(out, ref)


# --------------------------------------------------------------------------- 9. truncated publication
def truncated_runs(dev, to_dev):
    """unordered_knn on 3 loopback ranks whose trees (depth 7) are deeper than the published
    levels: the published leaves are inner nodes. Returns {levels: (distances, halo_recv)}."""
    p = clustered(20_000, seed=9)
    res = {}
    for levels in (2, 0):
        cfg = E.KnnConfig(k=16, publish_levels=levels)
        infos = [PL.RunInfo(PL.PhaseTimer(False, dev)) for _ in range(3)]

        def fn(comm):
            b, e = 20_000 * comm.rank // 3, 20_000 * (comm.rank + 1) // 3
            return PL.unordered_knn(to_dev(p[b:e]), comm, cfg, infos[comm.rank]).cpu()

        out = torch.cat(run_loopback(3, fn, dev))
        res[levels] = (out, sum(int(i.counts["halo_recv"]) for i in infos))
    return p, res


def test_truncated_publication_cpu():
    p, res = truncated_runs(torch.device(CPU), lambda t: t)
    ref = K.finalize_distances(K.kth_cpu(p, p, 16, math.inf))
    assert torch.equal(res[2][0], ref) and torch.equal(res[0][0], ref)
    print("halo_recv at 2 / 0 levels:", res[2][1], res[0][1])
    assert 0 < res[2][1] <= res[0][1]  # finer published leaves can only drop points
