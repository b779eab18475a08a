"""Edges of the grid kernel's cell stream (knn_grid.hip process_cell_stream): segment
lengths around the 8-candidate batch, one-grandchild segments, runs that end at slot 63 or
start at slot 0 of a cell, the segment that ends at the last sorted point (the read into
the pad), a long segment streamed in pieces of kSegCheck, a cutoff, the failure list and
the two-source and strided forms. Every GPU case compares the forced-grid k-th distances
bit for bit with the CPU oracle.

The sets are lattices inside chosen grandchild cells (level 5: 32 quanta of the 1024-quanta
cube per axis; cells of level 3 hold 64 of them), between two anchor points at the cube's
corners so that a lattice coordinate (q + 0.5) / 1024 quantises to exactly q. What a set
holds is checked on the CPU against the plain references of index_ref.py: a GPU pass over
a set that does not hold the intended runs would prove nothing.
"""
import math

import numpy as np
import pytest
import torch

import index_ref as R
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

gpu = pytest.mark.gpu
DEV = "cuda"
G = 5                      # grandchild level of every set here (forced: grid_level=G)
QG = 1024 >> G             # quanta per grandchild and axis
LENGTHS = (1, 7, 8, 9, 15, 16, 17)
SEG_CHECK = 1024           # knn_grid.hip kSegCheck
# 64 lattice offsets (in quanta) inside a grandchild
OFFS = np.array([(2 + 7 * a, 2 + 7 * b, 2 + 7 * c) for a in range(4) for b in range(4) for c in range(4)])
ANCHORS = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])


def lattice(gc, count):
    """`count` <= 64 lattice points of grandchild gc = (x, y, z) in [0, 32)^3."""
    q = np.asarray(gc)[None, :] * QG + OFFS[:count]
    return torch.from_numpy(((q + 0.5) / 1024.0).astype(np.float32))


def assemble(parts, seed):
    """The parts and the two anchors, shuffled."""
    p = torch.cat([ANCHORS] + parts)
    return p[torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(seed))].contiguous()


def slot_table(p):
    """Reference slots of the set on the Z-order curve: (cell, slot, count) per populated
    grandchild — cell = Morton index of the level-3 cell, slot = the 6 key bits below it."""
    keys = R.u32(R.morton_keys_ref(p, R.bounds_ref(p)))
    kg = torch.sort(keys >> (3 * (10 - G))).values
    uniq, cnt = torch.unique_consecutive(kg, return_counts=True)
    return uniq >> 6, uniq & 63, cnt


def lone_lengths(p):
    """Populations of the grandchildren that are alone in their level-3 cell: such a cell's
    stream is one segment of exactly that length (empty slots add nothing to a run)."""
    cell, _, cnt = slot_table(p)
    ucell, per_cell = torch.unique_consecutive(cell, return_counts=True)
    alone = ucell[per_cell == 1]
    return set(cnt[torch.isin(cell, alone)].tolist())


def make_lengths_set(seed=1, trim=None):
    """~2e4 points: per target length 12 cells with one populated grandchild of that length,
    and 270 cells with six populated grandchildren whose lengths cycle through the targets."""
    rng = np.random.default_rng(seed)
    cells = [c for c in rng.permutation(512) if c not in (0, 511)]  # (the anchors' cells stay out)
    parts, j = [], 0
    for i, c in enumerate(cells[:len(LENGTHS) * 12 + 270]):
        cxyz = np.array([c & 7, (c >> 3) & 7, c >> 6]) * 4
        lone = i < len(LENGTHS) * 12
        for s in rng.permutation(64)[:1 if lone else 6]:
            n = LENGTHS[i % len(LENGTHS)] if lone else LENGTHS[j % len(LENGTHS)]
            j += 1
            parts.append(lattice(cxyz + np.array([s & 3, (s >> 2) & 3, s >> 4]), n))
    p = assemble(parts, seed)
    return p if trim is None else p[:p.shape[0] - (p.shape[0] - trim) % 8]


def make_slot_edge_set(seed=2):
    """Cells whose only populated grandchildren are (3, 3, 3) — slot 63 on the Z-order curve,
    the run's last slot — or (0, 0, 0) — slot 0, the run's first —, or both with the 62
    slots between them empty (one run over the whole cell), 9 or 17 points each."""
    rng = np.random.default_rng(seed)
    cells = [c for c in rng.permutation(512) if c not in (0, 511)][:300]
    parts = []
    for i, c in enumerate(cells):
        cxyz = np.array([c & 7, (c >> 3) & 7, c >> 6]) * 4
        n = (9, 17)[i & 1]
        if i % 3 != 0:
            parts.append(lattice(cxyz + 3, n))
        if i % 3 != 1:
            parts.append(lattice(cxyz, n))
    return assemble(parts, seed)


def make_alternating_set(seed=3):
    """A 4 x 4 x 4 block of cells with every slot populated 6, 0, 2, 6, 0, 2, ... along the
    Z-order: with a cull radius of about one grandchild, needed, empty and unneeded slots
    alternate inside a cell and most segments are one grandchild long."""
    parts = []
    for c in range(64):
        cxyz = (np.array([c & 3, (c >> 2) & 3, c >> 4]) + 2) * 4
        for s in range(64):
            n = (6, 0, 2)[s % 3]
            if n:
                parts.append(lattice(cxyz + np.array([(s >> 2) & 1 | (s >> 4) & 2, (s >> 1) & 1 | (s >> 3) & 2,
                                                      s & 1 | (s >> 2) & 2]), n))
    return assemble(parts, seed)


def make_crowded_set(seed=4):
    """The lengths set plus one grandchild with 3000 points: 2800 random ones and 200 exact
    copies of one point (the segment is streamed in pieces of kSegCheck; the copies close
    every bound of their wave at k = 100)."""
    g = torch.Generator().manual_seed(seed)
    gc = torch.tensor([17.0, 9.0, 22.0])
    crowd = (gc * QG + 0.5 + torch.rand((2800, 3), generator=g) * (QG - 1)) / 1024.0
    copies = ((gc * QG + 11.25) / 1024.0).expand(200, 3)
    p = torch.cat([make_lengths_set(seed), crowd, copies])
    return p[torch.randperm(p.shape[0], generator=g)].contiguous()


_SETS, _ORACLE = {}, {}
MAKERS = {"lengths": make_lengths_set, "slot_edges": make_slot_edge_set, "alternating": make_alternating_set,
          "crowded": make_crowded_set, "end_mult8": lambda: make_lengths_set(5, trim=0),
          "end_odd": lambda: make_lengths_set(5, trim=3)}


def the_set(name):
    if name not in _SETS:
        _SETS[name] = MAKERS[name]()
    return _SETS[name]


def oracle(name, k, max_radius=math.inf):
    key = (name, k, max_radius)
    if key not in _ORACLE:
        p = the_set(name)
        _ORACLE[key] = K.finalize_distances(K.kth_cpu(p, p, k, E.cut2_of(max_radius)))
    return _ORACLE[key]


def grid_knn(p, k, max_radius=math.inf, **query_args):
    old = E.GRID
    E.GRID = "on"
    try:
        idx = E.build_index(p.to(DEV), grid=True, grid_level=G)
        assert idx.grid is not None and idx.grid.level + 2 == G
        st = E.KnnStats()
        out = torch.empty(idx.n, dtype=torch.float32, device=DEV)
        E.query(idx, E.KnnConfig(k=k, max_radius=max_radius), E.radius_hint(idx.box, idx.n, k), stats=st,
                final_out=out, **query_args)
        return out.cpu(), idx, st
    finally:
        E.GRID = old


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# --------------------------------------------------------------------------- the sets (CPU)
def test_sets_quantise_as_intended():
    for name in MAKERS:
        p = the_set(name)
        box = R.bounds_ref(p)
        assert box.tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1024.0, 1.0], name
    assert 15_000 <= the_set("lengths").shape[0] <= 25_000


def test_lengths_set_holds_every_target_length():
    p = the_set("lengths")
    assert set(LENGTHS) <= lone_lengths(p)           # as a whole cell's only segment
    _, _, cnt = slot_table(p)
    assert set(LENGTHS) <= set(cnt.tolist())         # and among several slots of a cell


def test_slot_edge_set_holds_runs_at_slot_0_and_63():
    cell, slot, cnt = slot_table(the_set("slot_edges"))
    ucell, per_cell = torch.unique_consecutive(cell, return_counts=True)
    inner = ~torch.isin(cell, torch.tensor([0, 511]))
    assert set(slot[inner].tolist()) == {0, 63} and set(cnt[inner].tolist()) == {9, 17}
    kinds = {tuple(slot[cell == c].tolist()) for c in ucell.tolist() if c not in (0, 511)}
    assert kinds == {(0,), (63,), (0, 63)}


def test_alternating_set_alternates_along_the_curve():
    cell, slot, cnt = slot_table(the_set("alternating"))
    full = [c for c in torch.unique(cell).tolist() if int((cell == c).sum()) == 43]
    assert len(full) == 64
    for c in full[:4]:
        m = cell == c
        assert slot[m].tolist() == [s for s in range(64) if s % 3 != 1]
        assert cnt[m].tolist() == [(6, 0, 2)[s % 3] for s in range(64) if s % 3 != 1]


def test_crowded_set_holds_a_long_segment_with_copies():
    p = the_set("crowded")
    _, _, cnt = slot_table(p)
    assert int(cnt.max()) == 3000 > 2 * SEG_CHECK
    _, copies = torch.unique(p, dim=0, return_counts=True)
    assert int(copies.max()) == 200 and int((copies > 1).sum()) == 1


def test_end_sets_differ_in_the_last_batch():
    assert the_set("end_mult8").shape[0] % 8 == 0 and the_set("end_odd").shape[0] % 8 == 3
    for name in ("end_mult8", "end_odd"):
        # the last grandchild of the curve holds few points: its segment ends at n
        p = the_set(name)
        keys, _ = K.morton(p, R.bounds_ref(p))
        kg = torch.sort(R.u32(keys) >> (3 * (10 - G))).values
        assert 1 <= int((kg == kg[-1]).sum()) <= 17


# --------------------------------------------------------------------------- the stream (GPU)
@gpu
@pytest.mark.parametrize("k", [1, 16, 100])
def test_segment_lengths_around_the_batch(k):
    got, _, st = grid_knn(the_set("lengths"), k)
    assert same_bits(got, oracle("lengths", k)), st.counters


@gpu
@pytest.mark.parametrize("k", [1, 16, 100])
def test_runs_ending_at_slot_63_and_starting_at_slot_0(k, monkeypatch):
    monkeypatch.setattr(K, "CURVE", "morton")  # (slot = Z-order rank: what the CPU check pinned)
    got, _, st = grid_knn(the_set("slot_edges"), k)
    assert same_bits(got, oracle("slot_edges", k)), st.counters


@gpu
@pytest.mark.parametrize("curve", ["morton", "hilbert"])
@pytest.mark.parametrize("k", [1, 16, 100])
def test_alternating_needed_empty_unneeded_slots(k, curve, monkeypatch):
    monkeypatch.setattr(K, "CURVE", curve)
    got, _, st = grid_knn(the_set("alternating"), k)
    assert same_bits(got, oracle("alternating", k)), st.counters
    assert st.counters.get("segments", 1) > 0


@gpu
@pytest.mark.parametrize("name", ["end_mult8", "end_odd"])
@pytest.mark.parametrize("k", [1, 16, 100])
def test_segment_ending_at_the_last_sorted_point(k, name):
    got, _, st = grid_knn(the_set(name), k)
    assert same_bits(got, oracle(name, k)), st.counters


@gpu
def test_long_segment_crosses_the_check():
    got, _, st = grid_knn(the_set("crowded"), 100)
    assert same_bits(got, oracle("crowded", 100)), st.counters
    # the copies' k-th neighbour is a copy
    p = the_set("crowded")
    _, inv, copies = torch.unique(p, dim=0, return_inverse=True, return_counts=True)
    assert bool((got[copies[inv] == 200] == 0).all())


@gpu
@pytest.mark.parametrize("k", [16, 100])
def test_cutoff_radius(k):
    for r in (0.004, 0.05):
        got, _, st = grid_knn(the_set("lengths"), k, r)
        assert same_bits(got, oracle("lengths", k, r)), (r, st.counters)


@gpu
@pytest.mark.parametrize("mod", [1, 7])
def test_failure_list_and_backstop(mod, monkeypatch):
    monkeypatch.setattr(E, "DEBUG_FAIL_MOD", mod)
    got, _, st = grid_knn(the_set("lengths"), 16)
    assert same_bits(got, oracle("lengths", 16)), st.counters
    assert st.counters.get("failed_lanes", 0) > 0


@gpu
def test_strided_persistent_form():
    """Every group listed, through the device-counted list in the persistent strided form."""
    k = 16
    p = the_set("lengths")
    old = E.GRID
    E.GRID = "on"
    try:
        idx = E.build_index(p.to(DEV), grid=True, grid_level=G)
        ng = (idx.n + 63) // 64
        groups = torch.arange(ng, dtype=torch.int32, device=DEV)
        cnt = torch.tensor([ng], dtype=torch.int32, device=DEV)
        d2 = torch.full((idx.n,), -7.0, device=DEV)
        E.query(idx, E.KnnConfig(k=k), E.radius_hint(idx.box, idx.n, k), out=d2, groups=groups, ngroups=ng,
                ngroups_dev=cnt, short_list=True)
        ref = K.kth_cpu(p, idx.pts[:idx.n].cpu(), k, math.inf)
        assert same_bits(d2.cpu(), ref)
    finally:
        E.GRID = old


@gpu
@pytest.mark.parametrize("k", [16, 100])
def test_two_source_form(k):
    """knn_grid2: the lengths set as the local points, the slot-edge set moved beside it as
    the halo (its own grid at the same level), the local k-th as the upper bound."""
    p = the_set("lengths")
    h = the_set("slot_edges") * 0.5 + torch.tensor([0.75, 0.25, 0.25])
    old = E.GRID
    E.GRID = "on"
    try:
        cfg = E.KnnConfig(k=k)
        idx = E.build_index(p.to(DEV), grid=True, grid_level=G)
        hidx = E.build_index(h.to(DEV), grid=True, grid_level=G, grid_gated=False)
        hint = E.radius_hint(idx.box, idx.n, k)
        d2 = E.query(idx, cfg, hint)
        ng = (idx.n + 63) // 64
        groups = torch.arange(ng, dtype=torch.int32, device=DEV)
        cnt = torch.tensor([ng], dtype=torch.int32, device=DEV)
        out = d2.clone()
        E.query(idx, cfg, hint, extra=hidx, groups=groups, ngroups=ng, ngroups_dev=cnt, short_list=True, out=out,
                init_d2=d2.clone())
        ref = K.kth_cpu(torch.cat([p, h]), idx.pts[:idx.n].cpu(), k, math.inf)
        assert same_bits(out.cpu(), ref)
    finally:
        E.GRID = old
