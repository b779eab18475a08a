"""The halo-filter, partition and result-return kernels (halo.hip, tree.hip, util.hip)
against the plain references of halo_ref.py: box tests within the float64 bracket
(must <= got <= may) and bit-equal to their CPU twins, everything else exact."""
import math

import pytest
import torch

import halo_ref as R
import test_halo_cpu as TC
from datasets import uniform
from mpi_cuda_largescaleknn_amd import _native
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.parallel import pipelines as PL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GPU = "cuda:0"


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def sentinel(n, dtype=torch.int32):
    return torch.full((n,), R.SENTINEL, dtype=dtype, device=DEV)


# --------------------------------------------------------------------------- 1. tree_set_radii
@pytest.mark.parametrize("mode", ["all", "last"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 4097, 10_000])
def test_tree_set_radii(n, mode):
    d2 = R.radii_case(n, mode)
    nodes = R.sentinel_nodes(n)
    ref = R.ref_tree_radii(nodes, n, d2)
    got = K.tree_set_radii(nodes.to(DEV), n, d2.to(DEV)).cpu()
    assert not bool(torch.isnan(got[1:, 3]).any())
    assert torch.equal(R.bits(got), R.bits(ref))          # radii, untouched columns, node 0
    slots, nb = nodes.shape[0] // 2, (n + 63) // 64
    assert float(got[slots + nb - 1, 3]) == math.inf      # the NaN of the last valid lane
    assert bool((got[slots + nb:, 3] == 0).all())         # leaf slots past the last bucket
    assert torch.equal(R.bits(got[0]), R.bits(nodes[0]))  # node 0: the radius hint
    assert torch.equal(R.bits(K.tree_set_radii(nodes.clone(), n, d2)), R.bits(got))  # CPU twin


# --------------------------------------------------------------------------- 2. halo_mask
def gpu_mask(pts, pub, offs, depths, self_rank):
    return K.halo_mask(pts.to(DEV), pub.reshape(-1).to(DEV), offs, depths, self_rank).cpu()


@pytest.mark.parametrize("variant", ["k8", "syn"])
@pytest.mark.parametrize("gen", R.GENS)
def test_halo_mask_bracket(gen, variant):
    S = R.shards(gen, GPU)
    pts = R.own_points(gen)
    share = R.Share()
    for depths in TC.DEPTH_MIXES:
        pub, offs, depths = R.publish(S.nodes(variant), depths, 6)
        must, may = R.mask_bracket(pts, pub, depths, 1, share)
        got = gpu_mask(pts, pub, offs, torch.tensor(depths, dtype=torch.int32, device=DEV), 1)
        R.assert_mask_in_bracket(got, must, may)
        assert bool((got & ~0b101 == 0).all())  # never the self bit, never a bit >= nranks
        assert torch.equal(got, TC.cpu_mask(pts, pub, offs, depths, 1))
    share.check(f"halo_mask {gen} {variant}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 9_477])
def test_halo_mask_sizes(n):
    """9 477 points: 38 blocks (no multiple of the 8 of xcd_remap), the last with empty waves."""
    S = R.shards("uniform", GPU)
    pts = R.own_points("uniform")[:n].contiguous()
    pub, offs, depths = R.publish(S.nodes("k8"), (0, 3, 6), 6)
    share = R.Share()
    must, may = R.mask_bracket(pts, pub, depths, 1, share)
    got = gpu_mask(pts, pub, offs, depths, 1)
    R.assert_mask_in_bracket(got, must, may)
    assert torch.equal(got, TC.cpu_mask(pts, pub, offs, depths, 1))
    share.check(f"halo_mask sizes n={n}")


@pytest.mark.parametrize("r2_other", [0.0, math.inf])
def test_halo_mask_hand_rows(r2_other):
    pts, in_quarter, in_zero, in_inf = R.hand_rows()
    box = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    pub, offs, depths = R.publish([R.one_leaf(*box, 0.25), R.one_leaf(*box, math.inf),
                                   R.one_leaf(*box, r2_other)], (0, 0, 0), 0)
    other = in_zero if r2_other == 0.0 else in_inf
    expect = torch.tensor([a | (b << 2) for a, b in zip(in_quarter, other)], dtype=torch.int64)
    got = gpu_mask(pts, pub, offs, depths, 1)
    assert torch.equal(got, expect)
    # the NaN rows (a NaN coordinate vanishes in fmaxf) are pinned to the CPU twin
    assert torch.equal(got, TC.cpu_mask(pts, pub, offs, depths, 1))


def test_halo_mask_padded_rows_never_hit():
    pts, in_quarter, _, _ = R.hand_rows()
    finite = ~torch.isnan(pts).any(1)
    for pad_r2 in (0.0, math.inf):
        nd = torch.zeros((4, 8))
        nd[:, 0:3], nd[:, 4:7] = math.inf, -math.inf
        nd[1] = R.one_leaf((0, 0, 0), (1, 1, 1), max(0.25, pad_r2))[1]
        nd[2] = R.one_leaf((0, 0, 0), (1, 1, 1), 0.25)[1]
        nd[3, 3] = pad_r2
        pub, offs, depths = R.publish([nd, nd], (1, 1), 1)
        got = gpu_mask(pts[finite].contiguous(), pub, offs, depths, 1)
        assert got.tolist() == [b for b, f in zip(in_quarter, finite.tolist()) if f]


def test_halo_mask_64_ranks():
    (pub, offs, depths), pts = TC.sixty_four_ranks()
    share = R.Share()
    must, may = R.mask_bracket(pts, pub, depths, 0, share)
    got = gpu_mask(pts, pub, offs, depths, 0)
    R.assert_mask_in_bracket(got, must, may)
    share.check("halo_mask 64 ranks")
    assert bool((got < 0).any()) and bool((got & 1 == 0).all())  # bit 63 works, no self bit
    assert torch.equal(got, TC.cpu_mask(pts, pub, offs, depths, 0))


def test_halo_mask_65_ranks_raises():
    nodes = [R.one_leaf((j, 0, 0), (j + 1, 1, 1), 0.01) for j in range(65)]
    pub, offs, depths = R.publish(nodes, [0] * 65, 0)
    with pytest.raises(_native.NativeError):
        gpu_mask(uniform(10), pub, offs, depths, 0)


# --------------------------------------------------------------------------- 3. mask_counts, halo_pack
@pytest.mark.parametrize("kind", ["random", "waves", "zero"])
@pytest.mark.parametrize("nranks", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 64, 65, 257, 10_000])
def test_mask_counts_and_pack(n, nranks, kind):
    lib = _native.hip()
    mask = R.random_masks(n, nranks, 5, kind)
    pts = uniform(n, seed=n)
    pts[0] = torch.tensor([math.nan, -0.0, 1.0])
    if n > 70:
        pts[70] = torch.tensor([-0.0, -0.0, -0.0])
    pop = R.bit_counts(mask, nranks)
    start = torch.arange(nranks, dtype=torch.int32) * 3 + 5
    counts = start.to(DEV)
    dmask, dpts = mask.to(DEV), pts.to(DEV)
    K.check(lib.lsk_hip_mask_counts(dmask.data_ptr(), n, nranks, counts.data_ptr(), stream()), "mask_counts")
    assert torch.equal(counts.cpu(), start + pop)
    # send ranges with two guard rows before, between and after them
    offs, o = [], 2
    for c in pop.tolist():
        offs.append(o)
        o += c + 2
    send = sentinel(3 * o).view(torch.float32).view(o, 3)
    cursors = torch.zeros(nranks, dtype=torch.int32, device=DEV)
    off_t = torch.tensor(offs, dtype=torch.int64, device=DEV)
    K.check(lib.lsk_hip_halo_pack(dpts.data_ptr(), dmask.data_ptr(), n, nranks, off_t.data_ptr(),
                                  cursors.data_ptr(), send.data_ptr(), stream()), "halo_pack")
    assert torch.equal(cursors.cpu(), pop)
    send = send.cpu()
    guard = torch.ones(o, dtype=torch.bool)
    for j, (off, c) in enumerate(zip(offs, pop.tolist())):
        guard[off:off + c] = False
        sel = ((mask >> j) & 1).bool()
        assert (R.sorted_rows(send[off:off + c]) == R.sorted_rows(pts[sel])).all()
    assert bool((R.bits(send)[guard] == R.SENTINEL).all())


# --------------------------------------------------------------------------- 4. compact_flags
@pytest.mark.parametrize("density", [0.0, 1.0 / 64.0, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 10_000])
def test_compact_flags(n, density):
    flags = R.flag_case(n, density)
    expect = torch.nonzero(flags).view(-1).to(torch.int32)
    lst = sentinel(n + 8)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    dflags = flags.to(DEV)
    K.check(_native.hip().lsk_hip_compact_flags(dflags.data_ptr(), n, lst.data_ptr(), cnt.data_ptr(), stream()),
            "compact_flags")
    c = int(cnt.item())
    assert c == expect.shape[0]
    assert torch.equal(torch.sort(lst[:c].cpu()).values, expect)
    assert bool((lst[c:].cpu() == R.SENTINEL).all())
    lst2, cnt2 = K.compact_flags(dflags)  # the wrapper, and its CPU twin
    assert int(cnt2.item()) == c and torch.equal(torch.sort(lst2[:c].cpu()).values, expect)


# --------------------------------------------------------------------------- 5. flag_groups_inverse
def flag_inverse(hpts, nh, nodes, depth, ngroups, flags):
    K.check(_native.hip().lsk_hip_flag_groups_inverse(hpts.data_ptr(), nh, nodes.data_ptr(), depth, ngroups,
                                                      flags.data_ptr(), stream()), "flag_groups_inverse")


def exact_flags_cpu(hpts, leaves):
    """The CPU halo_mask with every leaf as a one-leaf set of its own, 64 leaves per call:
    the canonical float32 test per (point, leaf) pair."""
    out = torch.zeros(leaves.shape[0], dtype=torch.bool)
    mask = torch.empty(hpts.shape[0], dtype=torch.int64)
    for s in range(0, leaves.shape[0], 64):
        lv = leaves[s:s + 64].contiguous()
        offs = torch.arange(lv.shape[0] + 1, dtype=torch.int64)
        _native.host().lsk_cpu_halo_mask(hpts.data_ptr(), hpts.shape[0], lv.data_ptr(), offs.data_ptr(),
                                         lv.shape[0], -1, mask.data_ptr(), 1)
        for b in range(lv.shape[0]):
            out[s + b] = bool(((mask >> b) & 1).any())
    return out


@pytest.mark.parametrize("variant", ["k8", "syn"])
@pytest.mark.parametrize("nh", [1, 64, 65, 5_000])
def test_flag_groups_inverse_bracket(nh, variant):
    S = R.shards("uniform", GPU)
    local = S.nodes(variant)[1]
    ng = (S.n[1] + 63) // 64
    assert ng < 64
    hpts = torch.cat([S.pts[2], S.pts[0].flip(0)])[:nh].contiguous()  # the neighbouring shards
    share = R.Share()
    leaves = local[64:64 + ng]
    mu, ma = R.bracket(R.point_gap2(hpts, leaves), leaves[None, :, 3])
    share.add(mu, ma)
    flags = sentinel(64 + 8)
    flags[:ng] = 0
    flags[3] = 1  # set already: stays set
    flag_inverse(hpts.to(DEV), nh, local.to(DEV), 6, ng, flags)
    got = flags.cpu()
    assert bool((got[ng:] == R.SENTINEL).all())          # nothing at or past ngroups
    assert bool(((got[:ng] == 0) | (got[:ng] == 1)).all()) and int(got[3]) == 1
    g = got[:ng].bool()
    g[3] = bool(exact_flags_cpu(hpts, leaves)[3])
    assert bool((mu.any(0) <= g).all()) and bool((g <= ma.any(0)).all())
    assert torch.equal(g, exact_flags_cpu(hpts, leaves))
    share.check(f"flag_groups_inverse {variant} nh={nh}")


def test_flag_groups_inverse_hand_rows_and_guards():
    pts, in_quarter, in_zero, in_inf = R.hand_rows()
    for r2, expect in ((0.25, in_quarter), (0.0, in_zero), (math.inf, in_inf)):
        nodes = R.one_leaf((0, 0, 0), (1, 1, 1), r2).to(DEV)
        for i, e in enumerate(expect):
            flags = sentinel(4)
            flags[0] = 0
            flag_inverse(pts[i:i + 1].contiguous().to(DEV), 1, nodes, 0, 1, flags)
            assert flags.cpu().tolist() == [e] + [R.SENTINEL] * 3, (r2, i)
    nodes = R.one_leaf((0, 0, 0), (1, 1, 1), math.inf).to(DEV)
    inside = torch.full((64, 3), 0.5, device=DEV)
    for nh, ng in ((0, 1), (64, 0)):  # nothing to do: the flags stay untouched
        flags = sentinel(4)
        flag_inverse(inside, nh, nodes, 0, ng, flags)
        assert bool((flags.cpu() == R.SENTINEL).all())
    with pytest.raises(_native.NativeError):
        flag_inverse(inside, 64, nodes, 31, 1, sentinel(4))


# --------------------------------------------------------------------------- 6. boundary_groups
@pytest.mark.parametrize("variant", ["ub", "syn"])
@pytest.mark.parametrize("ngroups", [1, 63, 65, 300])
def test_boundary_groups_bracket(ngroups, variant):
    local, depth = TC.local_tree(DEV, variant)
    assert depth == 9
    share = R.Share()
    for gen in ("uniform", "planar"):
        S = R.shards(gen, GPU)
        pub, offs, depths = R.publish(S.nodes("k8"), (0, 3, 6), 6)
        must, may = TC.boundary_bracket(local, depth, ngroups, pub, depths, 1, share)
        got = K.boundary_groups(local.to(DEV), depth, ngroups, pub.reshape(-1).to(DEV), offs, depths, 1).cpu()
        assert bool(((got == 0) | (got == 1)).all())
        assert bool((must <= got.bool()).all()) and bool((got.bool() <= may).all())
    share.check(f"boundary_groups {variant} {ngroups}")


def test_boundary_groups_depth0_local_tree_and_65_ranks():
    S = R.shards("uniform", GPU)
    share = R.Share()
    pub, offs, depths = R.publish(S.nodes("k8"), (3, 6, 0), 6)
    dpub = pub.reshape(-1).to(DEV)
    for r2 in (0.0, 1e-3, 0.3, math.inf):
        local = R.one_leaf((0.2, 0.2, 0.2), (0.25, 0.3, 0.3), r2)
        must, may = TC.boundary_bracket(local, 0, 1, pub, depths, 1, share)
        got = K.boundary_groups(local.to(DEV), 0, 1, dpub, offs, depths, 1).cpu().bool()
        assert bool((must <= got).all()) and bool((got <= may).all())
        assert bool(got[0]) == (r2 > 0.0)  # the box lies inside rank 0's slab: gap 0
    share.check("boundary_groups depth 0")
    with pytest.raises(_native.NativeError):
        K.boundary_groups(local.to(DEV), 0, 1, dpub, list(range(0, 65 * 16, 16)), [0] * 65, 1)


# --------------------------------------------------------------------------- 7. partition
@pytest.mark.parametrize("case", list(R.SPLITTER_CASES))
@pytest.mark.parametrize("n", [1, 1_023, 1_025, 300_001])
def test_dest_rank_and_perm(n, case):
    splitters = R.SPLITTER_CASES[case]
    keys = R.key_case(n, splitters)
    size = len(splitters) + 1
    ref = R.ref_dest(keys, splitters)
    dkeys = keys.to(DEV)
    split_t = torch.tensor(splitters if splitters else [0], dtype=torch.int32, device=DEV)
    dest, vals = sentinel(n + 4), sentinel(n + 4)
    K.check(_native.hip().lsk_hip_dest_rank(dkeys.data_ptr(), n, split_t.data_ptr(), len(splitters), R.SHIFT,
                                            dest.data_ptr(), vals.data_ptr(), stream()), "dest_rank")
    assert torch.equal(dest[:n].cpu(), ref)
    assert torch.equal(vals[:n].cpu(), torch.arange(n, dtype=torch.int32))
    assert bool((dest[n:].cpu() == R.SENTINEL).all()) and bool((vals[n:].cpu() == R.SENTINEL).all())
    perm, counts = PL._dest_and_perm(dkeys, splitters, size)
    assert torch.equal(perm.cpu().to(torch.int64), torch.sort(ref.to(torch.int64), stable=True).indices)
    assert torch.equal(counts.cpu().to(torch.int64), torch.bincount(ref.to(torch.int64), minlength=size))
    cperm, ccounts = PL._dest_and_perm(keys, splitters, size)
    assert torch.equal(perm.cpu(), cperm) and torch.equal(counts.cpu(), ccounts)


@pytest.mark.parametrize("sample", [1, 3, 7])
def test_key_histogram(sample):
    n = 100_003
    assert n % 3 and n % 7
    keys = R.key_case(n, [123, 40000])
    start = (torch.arange(1 << 16) % 5).to(torch.int32)
    hist = start.to(DEV)
    dkeys = keys.to(DEV)
    lib = _native.hip()
    K.check(lib.lsk_hip_key_histogram(dkeys.data_ptr(), n, R.SHIFT, sample, hist.data_ptr(), stream()),
            "key_histogram")
    ref = torch.bincount(keys[::sample].to(torch.int64) >> R.SHIFT, minlength=1 << 16).to(torch.int32)
    assert torch.equal(hist.cpu(), start + ref)
    with pytest.raises(_native.NativeError):
        K.check(lib.lsk_hip_key_histogram(dkeys.data_ptr(), n, R.SHIFT, 0, hist.data_ptr(), stream()),
                "key_histogram")


@pytest.mark.parametrize("ndest", [1, 3, 64, 1024])
def test_count_dest(ndest):
    n = 300_001
    g = torch.Generator().manual_seed(ndest)
    dest = torch.randint(0, ndest + 5, (n,), generator=g, dtype=torch.int32)
    dest[::1000] = -1  # 0xffffffff: far past ndest
    start = (torch.arange(ndest) % 7 + 1).to(torch.int32)
    counts = torch.cat([start, torch.full((8,), R.SENTINEL, dtype=torch.int32)]).to(DEV)
    ddest = dest.to(DEV)
    lib = _native.hip()
    K.check(lib.lsk_hip_count_dest(ddest.data_ptr(), n, ndest, counts.data_ptr(), stream()), "count_dest")
    inside = dest[(dest >= 0) & (dest < ndest)].to(torch.int64)
    assert torch.equal(counts[:ndest].cpu(), start + torch.bincount(inside, minlength=ndest).to(torch.int32))
    assert bool((counts[ndest:].cpu() == R.SENTINEL).all())  # entries >= ndest are ignored
    with pytest.raises(_native.NativeError):
        K.check(lib.lsk_hip_count_dest(ddest.data_ptr(), n, 1025, counts.data_ptr(), stream()), "count_dest")


# --------------------------------------------------------------------------- 8. scatter1, finalize
@pytest.mark.parametrize("n", [1, 257, 100_001])
def test_scatter1_finalize(n):
    d2 = R.d2_case(n)
    dd2 = d2.to(DEV)
    R.assert_same_floats(K.finalize_distances(dd2), R.ref_final(d2))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    dperm = perm.to(torch.int32).to(DEV)
    for fin in (False, True):
        out = torch.full((n + 3,), -7.0, device=DEV)
        K.scatter1(dd2, dperm, out, fin)
        ref = torch.full((n + 3,), -7.0)
        ref[perm] = R.ref_final(d2) if fin else d2
        R.assert_same_floats(out, ref)


# --------------------------------------------------------------------------- 9. truncated publication
def test_truncated_publication():
    p, res = TC.truncated_runs(DEV, lambda t: t.to(DEV))
    ref = E.knn_distances(p.to(DEV), 16).cpu()
    assert torch.equal(res[2][0], ref) and torch.equal(res[0][0], ref)
    print("halo_recv at 2 / 0 levels:", res[2][1], res[0][1])
    assert 0 < res[2][1] <= res[0][1]  # finer published leaves can only drop points
