"""Every recovery branch of the radix select of knn_rows.hip and knn_grid.hip, one input per
branch (select_ref.CASES), proven by the per-query status word:

  (a) reached: at least 16 queries carry the branch's bits, in the kernel the case forces;
  (b) resolved in place: none of them is handed to the exact backstop, and the call's
      fallback_queries is at most what the input must fail by construction (0 unless stated);
  (c) right: every distance of the case equals the brute-force host oracle bit for bit and
      lies in the float64 bracket of select_ref.kth_bracket.

Every case runs twice: outputs and masked status words are identical. The observed counts
stand next to each case (MI355X)."""
import math
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import select_ref as R
from datasets import GENERATORS
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
QS = R.status_bits["rows"]  # (the grid's values are the same where it has the bit)
MIN_REACHED = 16


def bits(*names):
    m = 0
    for nm in names:
        m |= QS["QS_" + nm]
    return m


@lru_cache(maxsize=None)
def _ref_rows(name):
    """Rows (of the input query array) the brute oracle is taken on: all of them, or for the
    two large inputs the rows that are not copies / not in the core plus 1000 of the rest."""
    p, q = R.case_input(name)
    nq = (q if q is not None else p).shape[0]
    if name == "walk":
        return torch.cat([torch.arange(64), 64 + torch.randperm(nq - 64, generator=torch.Generator().manual_seed(5))[:1000]])
    if name == "binwrap":
        ring = torch.nonzero((p != p.mode(dim=0).values).any(dim=1)).view(-1)
        rest = torch.nonzero((p == p.mode(dim=0).values).all(dim=1)).view(-1)
        return torch.cat([ring, rest[:1000]])
    return torch.arange(nq)


@lru_cache(maxsize=None)
def _oracle(name, k, cut2):
    """(rows, brute d² of those rows of the input query array): computed once per input."""
    p, q = R.case_input(name)
    rows = _ref_rows(name)
    return rows, K.kth_cpu(p, (q if q is not None else p)[rows].contiguous(), k, cut2, "brute")


def run_case(c, kern, cut2=math.inf, init_scale=None, init_bump=0):
    """One call on the forced kernel. Returns (dist float32 [nq] and masked status words
    int64 [nq], both in the order of the input query array, KnnStats)."""
    p, q = R.case_input(c.name)
    old = E.GRID
    E.GRID = "on" if kern == "grid" else "off"
    try:
        E.reset_kernels_used()
        idx = E.build_index(p.to(DEV), grid=True)
        assert (idx.grid is not None) == (kern == "grid")
        cfg = SimpleNamespace(k=c.k, cut2=cut2)  # (KnnConfig takes a radius: exact d² cutoffs need this)
        st = E.KnnStats()
        nq = (q if q is not None else p).shape[0]
        qs = torch.zeros(nq, dtype=torch.int32, device=DEV)
        if c.foreign:
            dist = E.query_points(idx, q.to(DEV), cfg, stats=st, qstatus=qs)
            # the status words are written at the curve-sorted query position
            qperm = E.prepare_queries(idx, q.to(DEV))[1].long()
            word = torch.empty_like(qs)
            word[qperm] = qs
        else:
            init = None
            if init_scale is not None:  # a known upper bound: scale x the true k-th d² (+ bump floats)
                rows, d2 = _oracle(c.name, c.k, math.inf)
                true = torch.empty(nq)
                true[rows] = d2
                ub = (true[idx.perm.cpu().long()] * init_scale).view(torch.int32) + init_bump
                init = ub.view(torch.float32).to(DEV)
            d2 = E.query(idx, cfg, E.radius_hint(idx.box, idx.n, c.k), stats=st, qstatus=qs, init_d2=init)
            # sorted position s holds input row perm[s]: back to input order
            perm = idx.perm.long()
            dist = torch.empty_like(d2)
            dist[perm] = K.finalize_distances(d2)
            word = torch.empty_like(qs)
            word[perm] = qs
        # (a pass with a known bound is a re-query: not recorded; without a grid it is knn_rows)
        assert E.kernels_used() == ([kern] if init_scale is None else [])
        return dist.cpu(), (word.cpu().to(torch.int64) & 0xFFFF), st
    finally:
        E.GRID = old


def check_right(c, dist, cut2=math.inf):
    """(c): bit-equal to the brute oracle and inside the float64 bracket, every reference row."""
    p, q = R.case_input(c.name)
    rows, d2 = _oracle(c.name, c.k, cut2)
    ref = K.finalize_distances(d2)
    got = dist[rows]
    bad = int((got.view(torch.int32) != ref.view(torch.int32)).sum())
    assert bad == 0, f"{bad} of {rows.numel()} rows differ from the brute oracle"
    qq = (q if q is not None else p)[rows]
    ok = R.kth_bracket(p, qq, got, c.k, cut2, count_fn=lambda a, b, v: R.bracket_counts_torch(a, b, v, DEV))
    assert ok.all(), f"{int((~ok).sum())} rows outside the float64 bracket"


def run_twice(c, kern, **kw):
    dist, word, st = run_case(c, kern, **kw)
    dist2, word2, _ = run_case(c, kern, **kw)
    assert torch.equal(dist.view(torch.int32), dist2.view(torch.int32)), "two runs differ in their outputs"
    assert torch.equal(word, word2), "two runs differ in their status words"
    return dist, word, st


def flagged(word, want, without=0):
    return ((word & want) == want) & ((word & without) == 0)


def report(c, kern, word, st, extra=""):
    vals, cnt = torch.unique(word, return_counts=True)
    top = sorted(zip(cnt.tolist(), vals.tolist()), reverse=True)[:10]
    keys = ("fallback_queries", "failed_lanes", "overflow_lanes", "underflow_lanes", "refine_lanes", "hint_lanes",
            "binovf_lanes", "mismatch_lanes", "pass_limit_waves", "list_invalid_waves", "guard_trips", "hist_passes",
            "waves")
    print(f"[select-paths] {R.case_id(c)} {kern} {extra} words(count, value)={top} "
          f"{ {k: st.counters.get(k, 0) for k in keys} }")


def test_status_bits_match_the_enums():
    for kern in ("rows", "grid"):
        assert R.parse_status_enum(kern) == R.status_bits[kern], kern


# One entry per branch that resolves in place: the bits at least MIN_REACHED queries carry
# (want), bits none of them may carry (without), and what the distances must be. Observed on
# an MI355X (flagged queries rows / grid, of nq):
#   overflow-k100    7200 / 1584 of 7200    300 clumps of 24, radius 1e-4
#   zero_fail-k16   24000 / 24000 of 24000  2000 sites x 12: probe of the zero bin, then the estimate's range
#   zero_fail-k100  24000 / 24000
#   zero_ok-k100    20000 / 20000 of 20000  100 sites x 200: one pass per wave
#   underflow1-k16     34 / 4002 of 8000    4000 in a 1e-2 cube + 4000 in the unit cube
#   underflow2-k16    951 / 1000 of 1000    foreign queries on 1000 sites x 20 (rows: the other 49 lie in
#                                           their group's located bucket and take the zero probe)
#   band1-k7, k27       0 / 0    of 4096    lattice(16): six (twenty) ties fit the pool share of 20 values per
#                                           lane, the band is collected, no one-bit band: COLLECTED asserted
#   ties-k100       16384 / 16384 of 16384  512 lattice sites x 32: 192 equal values exceed the pool share,
#                                           refines down to single-float bins end in the one-bit band
#   refine-k250        64 / 64   of 64      shell of 4000 at 0.97..1.03 around 200 points + 64 queries
#   crowd_hi-k16      512 (rows only) of 512  shell of 6000 at 0.94..1.06 inside sparse far data: LIST_INVALID
#                                           without OVERFLOW is set by a crowded-bin abort alone
#   crowd_lo-k16       24 (rows only) of 128  the same shell; the 24 queries at its centre share their groups with
#                                           104 decoy queries 50 away, so the located bucket (the median
#                                           query's) is far and the first range starts above the shell: crowded
#                                           bin 0 with an unknown base, the REFINE | UNDERFLOW restart (without
#                                           decoys the located bucket holds shell points: 7 of 64, 0 of 512)
#   hint-k100       19200 (rows) of 19200   300 sites x 64. knn_grid has no such branch: it takes no estimate
#                                           and sets HINT for every query of every input, so on the grid
#                                           only (b) and (c) are asserted for this input
#   tiny-k100, k101   n = 100: k == n finite, k > n the cutoff (inf)
SPEC = {
    "overflow-k100": dict(want=("OVERFLOW",)),
    "zero_fail-k16": dict(want=("OVERFLOW",), dist="positive"),
    "zero_fail-k100": dict(want=("OVERFLOW",), dist="positive"),
    "zero_ok-k100": dict(want=("DONE_BAND1",), without=("OVERFLOW", "UNDERFLOW", "REFINE"), dist="zero", one_pass=True),
    "underflow1-k16": dict(want=("UNDERFLOW",)),
    "underflow2-k16": dict(want=("UNDERFLOW",), dist="zero"),
    "band1-k7": dict(want=("COLLECTED",), without=("DONE_BAND1", "REFINE")),
    "band1-k27": dict(want=("COLLECTED",), without=("DONE_BAND1", "REFINE")),
    "ties-k100": dict(want=("DONE_BAND1", "REFINE")),
    "refine-k250": dict(want=("REFINE",)),
    "crowd_hi-k16": dict(want=("REFINE", "LIST_INVALID"), without=("OVERFLOW", "UNDERFLOW")),
    "crowd_lo-k16": dict(want=("REFINE", "UNDERFLOW", "LIST_INVALID"), without=("OVERFLOW",)),
    "hint-k100": dict(want=("HINT",)),
    "tiny-k100": dict(want=(), dist="finite"),
    "tiny-k101": dict(want=("DONE_CUT",), dist="inf"),
}
IN_PLACE = [(c, kern) for c in R.CASES if R.case_id(c) in SPEC for kern in c.kernels]


@pytest.mark.parametrize("c,kern", IN_PLACE, ids=[f"{R.case_id(c)}-{kern}" for c, kern in IN_PLACE])
def test_branch_reached_and_resolved_in_place(c, kern):
    spec = SPEC[R.case_id(c)]
    if c.name == "hint" and kern == "grid":
        spec = dict(want=())  # (HINT is unconditional in knn_grid: nothing to reach)
    dist, word, st = run_twice(c, kern)
    hit = flagged(word, bits(*spec["want"]), bits(*spec.get("without", ())))
    report(c, kern, word, st, f"flagged={int(hit.sum())}")
    assert int(hit.sum()) >= MIN_REACHED, "(a) branch not reached"
    assert int((word[hit] & bits("FAIL")).ne(0).sum()) == 0, "(b) flagged queries went to the backstop"
    assert st.counters["fallback_queries"] == 0 and st.counters["failed_lanes"] == 0, st.counters
    assert st.counters["pass_limit_waves"] == 0 and st.counters["mismatch_lanes"] == 0
    check_right(c, dist)
    want = spec.get("dist")
    if want == "zero":
        assert bool((dist[hit] == 0).all())
    elif want == "positive":
        assert bool((dist[hit] > 0).all())
    elif want == "finite":
        assert bool(torch.isfinite(dist).all())
    elif want == "inf":
        assert bool(torch.isinf(dist).all())
    if spec.get("one_pass"):
        # the probe's bin 0 holds k zeros in the first pass: one histogram pass per wave
        assert st.counters["hist_passes"] == st.counters["waves"]


@pytest.mark.parametrize("kern", ["rows", "grid"])
def test_bin_wrap_goes_to_the_backstop(kern):
    """70 000 copies of A and 64 ring points at nearly one distance from it, k = 100: every
    ring query sees 70 000 equal values. MI355X, of 70 064 queries:
    rows: crowded-bin restarts refine to single-float bins, then a pass over all copies costs
      4375 of the wave's 8192 row-steps: the wrap is caught for 4 ring queries (BINOVF), the walk
      budget stops the other 60 first (guard_trips 2); 68 queries fail (64 + 4 copies of A in
      the ring's waves) and are exact through the backstop.
    grid: 52 queries BINOVF (4 ring, 48 copies next to them), 60 ring queries over the candidate
      budget (FAIL without BINOVF); 112 fail.
    Must-fail = the flagged queries: fallback_queries equals the number of FAIL words."""
    c = next(x for x in R.CASES if x.name == "binwrap")
    dist, word, st = run_twice(c, kern)
    rows, _ = _oracle(c.name, c.k, math.inf)
    ring = rows[:64]
    fail = (word & bits("FAIL")) != 0
    wrap = flagged(word, bits("BINOVF"))
    report(c, kern, word, st, f"fail={int(fail.sum())} binovf={int(wrap.sum())}")
    assert bool(fail[ring].all()), "a ring query resolved 70 000 equal values in 16-bit bins"
    assert bool(fail[wrap].all())
    if kern == "grid":
        assert int(wrap.sum()) >= MIN_REACHED
    else:  # the walk budget pre-empts the wrap for most ring queries: one of the two, every one
        assert int(wrap.sum()) >= 1 and st.counters["guard_trips"] > 0
    assert st.counters["binovf_lanes"] == int(wrap.sum())
    assert st.counters["fallback_queries"] == int(fail.sum()) == st.counters["failed_lanes"]
    assert int(fail.sum()) <= 128  # the ring's waves, nothing else
    assert st.counters["pass_limit_waves"] == 0 and st.counters["mismatch_lanes"] == 0
    copies = torch.ones(word.numel(), dtype=torch.bool)
    copies[ring] = False
    assert bool((dist[copies] == 0).all())
    check_right(c, dist)


@pytest.mark.parametrize("kern", ["rows", "grid"])
def test_walk_budget_goes_to_the_backstop(kern):
    """300 000 points in a 1e-3 cube and 64 sparse points at distance 0.8..1.2 whose 100th
    neighbour lies in the cube (the one large case; the brute reference covers the sparse
    points and 1000 of the core). MI355X:
    rows: guard_trips 4, 96 queries fail (the 64 sparse ones and core points sharing their waves).
    grid: forced onto this input the grid gives up on every wave (a range it cannot serve or the
      candidate budget): all 300 064 words are FAIL | HINT, the designed answer of a forced grid,
      and the backstop serves the whole set."""
    c = next(x for x in R.CASES if x.name == "walk")
    dist, word, st = run_twice(c, kern)
    fail = (word & bits("FAIL")) != 0
    report(c, kern, word, st, f"fail={int(fail.sum())}")
    sparse = torch.arange(64)
    assert bool(fail[sparse].all())
    if kern == "grid":
        assert int((word[sparse] & bits("BINOVF", "LIMIT", "MISMATCH")).ne(0).sum()) == 0
    else:  # (a truncated walk's collect count is partial: MISMATCH next to FAIL there is no finding)
        assert st.counters["guard_trips"] > 0
        assert int((word[sparse] & bits("BINOVF", "LIMIT")).ne(0).sum()) == 0
        assert int(fail.sum()) <= 64 * 64  # at most the waves that hold a sparse point
    assert st.counters["fallback_queries"] == int(fail.sum()) == st.counters["failed_lanes"]
    assert st.counters["pass_limit_waves"] == 0 and st.counters["mismatch_lanes"] == 0
    check_right(c, dist)


UNIFORM = next(x for x in R.CASES if x.name == "uniform")


@lru_cache(maxsize=None)
def _unbounded_uniform():
    """The same pass without a bound: (status words, counters), the baseline of the bound's effect."""
    _, word, st = run_case(UNIFORM, "rows")
    return word, dict(st.counters)


@pytest.mark.parametrize("scale,bump", [(1.0, 0), (1.0, 1), (1.5, 0), (64.0, 0)])
def test_known_upper_bound_never_overflows(scale, bump):
    """init_d2 = scale x the true k-th d² (+ bump floats): the first range ends just above the
    bound, so no query overflows, whether the bound is the true value itself, one float above
    it, loose or very loose. (The single-index form with a bound runs on knn_rows.)
    That the bound is used shows against the same pass without one, which neither overflows nor
    underflows on this input. A tight bound (<= 1.5 x) closes the walk's radius from the first
    candidate on: the first range's top is the bound, below the estimate's top for most queries,
    and the walk order is the same, so the pass evaluates fewer candidates. A bound 64 x too
    large puts the k-th six octaves below the range's top, one more than the range spans: every
    query takes the underflow restart. MI355X, evals: no bound 323808; 1 x and 1 x + one float 285664; 1.5 x 309424; 64 x 562272
    with 20 000 of 20 000 queries UNDERFLOW."""
    base_word, base = _unbounded_uniform()
    assert int(flagged(base_word, bits("OVERFLOW")).sum()) == 0 and int(flagged(base_word, bits("UNDERFLOW")).sum()) == 0
    dist, word, st = run_twice(UNIFORM, "rows", init_scale=scale, init_bump=bump)
    report(UNIFORM, "rows", word, st, f"scale={scale} bump={bump} evals={st.counters['evals']} (no bound {base['evals']})")
    assert int(flagged(word, bits("OVERFLOW")).sum()) == 0
    assert int(flagged(word, bits("HINT")).sum()) == 0
    if scale <= 1.5:
        assert st.counters["evals"] < base["evals"]
        assert int(flagged(word, bits("UNDERFLOW")).sum()) == 0
    else:
        assert int(flagged(word, bits("UNDERFLOW")).sum()) == word.numel()
    assert st.counters["fallback_queries"] == 0 and st.counters["failed_lanes"] == 0
    check_right(UNIFORM, dist)


@pytest.mark.parametrize("kern", ["rows", "grid"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_cutoff_exits(kern, which):
    """Cutoffs at the true k-th d² of one query, one float above it and one float below it
    (which 0, 1, 2): every query whose k-th
    lies at or above the cutoff (strict <, as the oracle) leaves through DONE_CUT with the
    cutoff as its answer, the others below it are untouched. About half the queries each."""
    cut2 = R.uniform_cutoffs(UNIFORM.k)[which]
    dist, word, st = run_twice(UNIFORM, kern, cut2=cut2)
    report(UNIFORM, kern, word, st, f"cut2={cut2!r}")
    fin = float(np.sqrt(np.float64(np.float32(cut2))).astype(np.float32))
    at_cut = dist == fin
    cut_bit = flagged(word, bits("DONE_CUT"))
    assert int(cut_bit.sum()) >= MIN_REACHED and int((~cut_bit).sum()) >= MIN_REACHED
    assert bool(at_cut[cut_bit].all())
    assert bool((dist <= fin).all())
    assert int((word & bits("FAIL")).ne(0).sum()) == 0 and st.counters["fallback_queries"] == 0
    check_right(UNIFORM, dist, cut2)
    # the query the cutoff was taken from: its own k-th is not < cut2 (which 0 and 2), is (which 1)
    _, d2 = _oracle(UNIFORM.name, UNIFORM.k, math.inf)
    own = torch.nonzero(d2 == np.float32(R.uniform_cutoffs(UNIFORM.k)[0])).view(-1)
    assert own.numel() >= 1
    if which != 1:  # (the grid clips a band that reaches past the cutoff at the end: same value, no bit)
        assert bool((dist[own] == fin).all()) and (kern == "grid" or bool(cut_bit[own].all()))
    else:
        assert bool((dist[own] < fin).all()) and not bool(cut_bit[own].any())


@pytest.mark.parametrize("dist_name", ["uniform", "clustered", "planar", "duplicates"])
@pytest.mark.parametrize("k", [16, 100])
def test_no_query_needs_the_backstop(dist_name, k, monkeypatch):
    """Whole-suite guard at test_knn_matches_oracle's sizes, knn_rows: equality with the oracle
    also holds when a broken branch sends its queries to the exact backstop, so the counts of
    failed lanes, mismatches and pass-limit waves are pinned to 0 (fixed seeds: deterministic,
    run twice)."""
    monkeypatch.setattr(E, "GRID", "off")
    monkeypatch.setattr(E, "KNN_IMPL", "rows")
    p = GENERATORS[dist_name](30000, seed=k).to(DEV)
    seen = []
    for _ in range(2):
        st = E.KnnStats()
        E.reset_kernels_used()
        E.knn_distances(p, k, stats=st)
        assert E.kernels_used() == ["rows"]
        seen.append((st.counters["failed_lanes"], st.counters["mismatch_lanes"], st.counters["pass_limit_waves"],
                     st.counters["fallback_queries"]))
    print(f"[select-paths] guard {dist_name} k={k}: {seen}")
    assert seen[0] == seen[1] == (0, 0, 0, 0)
