"""Two-sided radius search on the host: the brute-force oracle K.radius_reach_count_cpu /
K.radius_reach_cpu bit for bit against the plain numpy reference of radius_reach_ref.py, the
identities that tie reach_* to the one-sided searches, the errors, the edge cases and the
hipKNN_radius --reach / lsknn_tools rcheck round trip. The conditions under which a case says
anything (a wrapped pair, rows that differ from the one-sided ones) are asserted from the
reference."""
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

import radius_reach_ref as R
import scale_cases as S
from datasets import clustered, duplicates, uniform
from mpi_cuda_largescaleknn_amd.apps import radius as radius_app
from mpi_cuda_largescaleknn_amd.apps import tools
from mpi_cuda_largescaleknn_amd.models import knn_engine as E
from mpi_cuda_largescaleknn_amd.ops import kernels as K
from mpi_cuda_largescaleknn_amd.utils import io

INF = math.inf
RULES = ("either", "both")
DATA = {"uniform": uniform, "clustered": clustered, "duplicates": duplicates}
PERIODS = {"open": None, "L1": 1.0, "L1x0.7xinf": (1.0, 0.7, INF)}


def bound_of(period) -> float:
    """The largest radius of a case: the period's bound, 0.5 in the open box."""
    if period is None:
        return 0.5
    return E.period_radius_bound(K.check_period("test", period), False)


def reach_radii(m: int, top: float, seed: int) -> torch.Tensor:
    """Log-uniform over two decades up to `top`, three entries at 0 and three at exactly `top`."""
    g = torch.Generator().manual_seed(seed)
    r = torch.exp(math.log(top / 100.0) + math.log(100.0) * torch.rand(m, generator=g)).float().clamp(max=top)
    where = torch.randperm(m, generator=g)
    r[where[:3]] = 0.0
    r[where[3:6]] = top
    return r.contiguous()


def case(name: str, pname: str, n: int = 700, nq: int = 500):
    period = PERIODS[pname]
    p = DATA[name](n, seed=3)
    q = (DATA[name](nq, seed=4) * 1.1 - 0.05).contiguous()
    top = bound_of(period)
    return p, q, reach_radii(nq, top, 5), reach_radii(n, top, 6), period


def csr(lists):
    return tuple(t.numpy() if torch.is_tensor(t) else t for t in lists)


def same_csr(got, ref) -> bool:
    """(offsets, idx, d2 or dist): equal ids and equal bits."""
    g, w = csr(got), csr(ref)
    return np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) \
        and np.array_equal(g[2].view(np.uint32), w[2].view(np.uint32))


def rows(lists) -> list:
    o, i, d = csr(lists)
    return [list(zip(i[o[r]:o[r + 1]].tolist(), d[o[r]:o[r + 1]].view(np.uint32).tolist())) for r in range(o.size - 1)]


def conditions(p, q, qc, pc, rule, period):
    """What makes a case say something, from the reference alone."""
    m, _ = R.selected(p, q, qc, pc, rule, period)
    zq, zp = np.zeros(q.shape[0], np.float32), np.zeros(p.shape[0], np.float32)
    gather, _ = R.selected(p, q, qc, zp, "either", period)
    scatter, _ = R.selected(p, q, zq, pc, "either", period)
    if period is not None and any(math.isfinite(v) for v in R.as_period(period)):
        assert (m & R.wraps(p, q, period)).any(), "no selected pair wraps"
    if rule == "either":
        assert (m != gather).any(1).any() and (m != scatter).any(1).any()
    else:
        c = m.sum(1)
        assert (c > 0).any() and ((c < gather.sum(1)) & (c < scatter.sum(1))).any()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("pname", sorted(PERIODS))
@pytest.mark.parametrize("name", sorted(DATA))
def test_oracle_against_the_reference(name, pname, rule):
    p, q, rq, rp, period = case(name, pname)
    qc, pc = rq * rq, rp * rp
    conditions(p, q, qc, pc, rule, period)
    counts, offsets, idx, d2 = R.reach(p, q, qc, pc, rule, period)
    assert np.array_equal(K.radius_reach_count_cpu(p, q, qc, pc, rule, period).numpy(), counts)
    assert same_csr(K.radius_reach_cpu(p, q, qc, pc, rule, period), (offsets, idx, d2))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("origin", ["zero", "p1000"])
@pytest.mark.parametrize("pname", sorted(S.PERIODS))
def test_oracle_on_the_scale_periods(pname, origin, rule):
    n = nq = 400
    period = S.PERIODS[pname]
    p = S.periodic_points("uniform", n, pname, origin)
    q = S.periodic_points("clustered", nq, pname, origin, seed=1)
    top = S.period_radius(pname, 0.5)
    rq, rp = reach_radii(nq, top, 7), reach_radii(n, top, 8)
    qc, pc = rq * rq, rp * rp
    assert float(qc.max()) <= K.period_cut2_bound(K.check_period("test", period))
    conditions(p, q, qc, pc, rule, period)
    counts, offsets, idx, d2 = R.reach(p, q, qc, pc, rule, period)
    assert np.array_equal(K.radius_reach_count_cpu(p, q, qc, pc, rule, period).numpy(), counts)
    assert same_csr(K.radius_reach_cpu(p, q, qc, pc, rule, period), (offsets, idx, d2))
    # and the engine on a CPU index, radii as distances
    index = E.build_index(p)
    got = E.reach_neighbors(index, q, rq, rp, rule=rule, period=period)
    assert same_csr(got, (offsets, idx, K.finalize_distances(torch.from_numpy(d2))))
    assert np.array_equal(E.reach_counts(index, q, rq, rp, rule=rule, period=period).numpy(), counts)


@pytest.mark.parametrize("pname", sorted(PERIODS))
@pytest.mark.parametrize("name", sorted(DATA))
def test_identities(name, pname):
    p, q, rq, rp, period = case(name, pname)
    n, nq = p.shape[0], q.shape[0]
    qc, pc = rq * rq, rp * rp
    index = E.build_index(p)
    per = {} if period is None else {"period": period}
    either = E.reach_neighbors(index, q, rq, rp, **per)
    both = E.reach_neighbors(index, q, rq, rp, rule="both", **per)
    gather = E.radius_neighbors(index, q, rq, **per)
    # zero point radii: the gather search; query_radii = 0.0: the scatter search
    assert same_csr(E.reach_neighbors(index, q, rq, torch.zeros(n), **per), gather)
    assert torch.equal(E.reach_counts(index, q, rq, torch.zeros(n), **per), E.radius_counts(index, q, rq, **per))
    scatter = E.reach_neighbors(index, q, 0.0, rp, **per)
    if period is None:
        assert same_csr(scatter, E.point_radius_neighbors(index, q, rp))
        assert torch.equal(E.reach_counts(index, q, 0.0, rp), E.point_radius_counts(index, q, rp))
        assert same_csr(K.radius_reach_cpu(p, q, qc, pc, "both"), K.radius_var_cpu(p, q, qc, pc))
        assert torch.equal(K.radius_reach_count_cpu(p, q, qc, pc, "both"), K.radius_var_count_cpu(p, q, qc, pc))
        # an all-open period: the open result
        for rule, ref in (("either", either), ("both", both)):
            assert same_csr(E.reach_neighbors(index, q, rq, rp, rule=rule, period=(INF,) * 3), ref)
            assert same_csr(K.radius_reach_cpu(p, q, qc, pc, rule, (INF,) * 3), K.radius_reach_cpu(p, q, qc, pc, rule))
    # equal constant radii on both sides: radius_neighbors(r) under both rules
    r = 0.3 * bound_of(period)
    const = E.radius_neighbors(index, q, r, **per)
    for rule in RULES:
        assert same_csr(E.reach_neighbors(index, q, r, torch.full((n,), r), rule=rule, **per), const)
        assert same_csr(E.reach_neighbors(index, q, torch.full((nq,), r), torch.full((n,), r), rule=rule, **per), const)
    # rows: either = the sorted union, both = the intersection of the gather and the scatter row
    # (on the oracle's d2 bits, the sort key: final distances may tie where d2 does not)
    zq, zp = torch.zeros(nq), torch.zeros(n)
    d2_lists = [K.radius_reach_cpu(p, q, a, b, rule, period)
                for a, b, rule in ((qc, pc, "either"), (qc, pc, "both"), (qc, zp, "either"), (zq, pc, "either"))]
    for got, ref in zip((either, both, gather, scatter), d2_lists):
        assert same_csr(got, (ref[0], ref[1], K.finalize_distances(ref[2])))
    for e, b, g, s in zip(*(rows(t) for t in d2_lists)):
        assert e == sorted(set(g) | set(s), key=lambda t: (t[1], t[0]))
        assert b == sorted(set(g) & set(s), key=lambda t: (t[1], t[0]))
    # squared radii and the convenience forms
    assert same_csr(E.reach_neighbors(index, q, qc, pc, squared=True, **per), either)
    assert same_csr(E.reach_query_neighbors(p, q, rq, rp, rule="both", **per), both)
    assert torch.equal(E.reach_query_counts(p, q, rq, rp, **per), torch.from_numpy(np.diff(csr(either)[0])).int())
    assert same_csr(E.reach_neighbors(index, q, rq, E.prepare_point_radii(index, rp), **per), either)
    assert same_csr(by_id(E.reach_neighbors(index, q, rq, rp, sort=False, **per)), by_id(either))
    st = E.KnnStats()
    E.reach_counts(index, q, rq, rp, stats=st, **per)  # (a CPU index reports no counters)
    assert st.counters == {}


def by_id(lists):
    o, i, d = csr(lists)
    row = np.repeat(np.arange(o.size - 1), np.diff(o))
    order = np.lexsort((i, row))
    return o, i[order], d[order]


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("pname", sorted(PERIODS))
def test_self_neighbours_are_symmetric(pname, rule):
    period = PERIODS[pname]
    p = clustered(600, seed=9)
    h = reach_radii(600, bound_of(period), 10)
    conditions(p, p, h * h, h * h, rule, period)
    o, i, d = csr(E.reach_self_neighbors(p, h, rule=rule, period=period))
    row = np.repeat(np.arange(600), np.diff(o))
    fwd = set(zip(row.tolist(), i.tolist(), d.view(np.uint32).tolist()))
    assert len(fwd) == i.size > 600
    assert fwd == {(b, a, w) for a, b, w in fwd}


def test_edge_cases():
    p = uniform(500, seed=15)
    q = uniform(200, seed=16)
    q[3, 1] = math.nan
    q[40] = math.nan
    q[77, 0] = INF
    rq, rp = reach_radii(200, 0.4, 17), reach_radii(500, 0.4, 18)
    rq[5] = rq[3] = INF
    rp[9] = INF
    index = E.build_index(p)
    for rule in RULES:
        got = E.reach_neighbors(index, q, rq, rp, rule=rule)
        ref = R.reach(p, q, rq * rq, rp * rp, rule)
        assert same_csr(got, (ref[1], ref[2], K.finalize_distances(torch.from_numpy(ref[3]))))
        c = np.diff(csr(got)[0])
        assert c[3] == 0 and c[40] == 0 and c[77] == 0
        # an infinite query radius: every point, or under "both" the scatter search alone
        assert c[5] == (500 if rule == "either" else int(K.radius_var_count_cpu(p, q[5:6], None, rp * rp)[0]))
        zero_q = (rq == 0).nonzero().flatten().tolist()
        if rule == "both":
            assert all(c[z] == 0 for z in zero_q)
            assert not np.isin(csr(got)[1], (rp == 0).nonzero().flatten().numpy()).any()
        else:  # reached by the point of infinite radius at least
            assert all(c[z] >= 1 for z in zero_q)
            assert all(9 in [t[0] for t in r] for k, r in enumerate(rows(got)) if k not in (3, 40, 77))
    # nothing to search, nothing to ask
    none, no_r = torch.empty((0, 3)), torch.empty(0)
    for rule in RULES:
        assert E.reach_counts(index, none, no_r, rp, rule=rule).shape == (0,)
        o, i, d = E.reach_neighbors(index, none, 0.1, rp.clamp(max=0.5), rule=rule, period=1.0)
        assert torch.equal(o, torch.zeros(1, dtype=torch.int64)) and i.numel() == 0 and d.numel() == 0
        assert torch.equal(E.reach_query_counts(none, q, rq, no_r, rule=rule), torch.zeros(200, dtype=torch.int32))
        o, i, d = E.reach_query_neighbors(none, q, rq, no_r, rule=rule)
        assert torch.equal(o, torch.zeros(201, dtype=torch.int64)) and i.numel() == 0 and d.numel() == 0
    # max_pairs: the total itself passes, one less raises before the lists exist
    total = int(E.reach_counts(index, q, rq, rp).sum())
    with pytest.raises(ValueError, match=str(total)):
        E.reach_neighbors(index, q, rq, rp, max_pairs=total - 1)
    assert E.reach_neighbors(index, q, rq, rp, max_pairs=total)[1].numel() == total


def test_errors(monkeypatch):
    p, q = uniform(300, seed=19), uniform(100, seed=20)
    index = E.build_index(p)
    rq, rp = torch.full((100,), 0.05), torch.full((300,), 0.05)

    def launched(*a, **k):
        raise AssertionError("a kernel ran")

    for name in ("radius_reach_count_cpu", "radius_reach_cpu", "radius_reach_count_gpu", "radius_reach_fill_gpu"):
        monkeypatch.setattr(K, name, launched)

    def variants(r):
        neg, nan = r.clone(), r.clone()
        neg[11], nan[11] = -0.5, math.nan
        return [neg, nan, r.double(), r[:-1], torch.cat([r, r[:1]]), r.view(-1, 1), "0.1", None]

    fns = (E.reach_counts, E.reach_neighbors)
    for fn in fns:
        for bad in variants(rq) + [-0.1, math.nan]:
            with pytest.raises(ValueError):
                fn(index, q, bad, rp)
        for bad in variants(rp) + [0.05]:
            with pytest.raises(ValueError):
                fn(index, q, rq, bad)
        for rule in ("any", "EITHER", "", None, 0):
            with pytest.raises(ValueError, match="rule"):
                fn(index, q, rq, rp, rule=rule)
        for period in (0.0, -1.0, math.nan, (1.0, 1.0), "x"):
            with pytest.raises(ValueError):
                fn(index, q, rq, rp, period=period)
        # above half the period: either side, tensor, number or prepared radii
        top = E.period_radius_bound((1.0, 0.7, INF), False)
        over = S.float_above(top)
        big_q, big_p = rq.clone(), rp.clone()
        big_q[50] = big_p[50] = over
        for a, b in ((big_q, rp), (rq, big_p), (over, rp), (rq, E.prepare_point_radii(index, big_p))):
            with pytest.raises(ValueError, match="period"):
                fn(index, q, a, b, period=(1.0, 0.7, INF))
        with pytest.raises(ValueError, match="period"):
            fn(index, q, rq * rq, big_p * big_p, squared=True, period=(1.0, 0.7, INF))
        with pytest.raises(ValueError, match="another index"):
            fn(index, q, rq, E.prepare_point_radii(E.build_index(p.clone()), rp))
        with pytest.raises(ValueError):
            fn(index, q[:, :2], rq, rp)
        with pytest.raises(ValueError):
            fn(index, q.double(), rq, rp)
    # an index in a rotated frame, or sorted by line keys
    # (a CPU index is never either: the fields alone are set here, the device test builds one)
    for odd in (dataclasses.replace(index, qrot=torch.eye(3)), dataclasses.replace(index, line=True)):
        for fn in fns:
            with pytest.raises(ValueError):
                fn(odd, q, rq, rp)
    monkeypatch.undo()
    # at the bound itself everything runs, and point_radius_* keeps its refusal
    top = E.period_radius_bound((1.0, 0.7, INF), False)
    at_q, at_p = rq.clone(), rp.clone()
    at_q[50] = at_p[50] = top
    assert int(E.reach_counts(index, q, at_q, at_p, period=(1.0, 0.7, INF)).sum()) > 0
    with pytest.raises(ValueError, match="not supported"):
        E.point_radius_counts(index, q, rp, period=1.0)


SUFFIXES = (".count", ".offsets", ".ids", ".dist")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("extra", [[], ["--rule", "both"], ["--period", "1"], ["--rule", "both", "--period", "1,0.7,inf"]],
                         ids=["either", "both", "either-L1", "both-L1x0.7xinf"])
def test_cli_round_trip(tmp_path, capsys, extra):
    p, q = uniform(1500, seed=11), uniform(400, seed=12)
    fp, fq = str(tmp_path / "p.float3"), str(tmp_path / "q.float3")
    frq, frp = str(tmp_path / "rq.float"), str(tmp_path / "rp.float")
    io.write_points(fp, p)
    io.write_points(fq, q)
    rq, rp = reach_radii(400, 0.35, 21), reach_radii(1500, 0.35, 22)
    io.write_array(frq, rq)
    io.write_array(frp, rp)
    rule = "both" if "--rule" in extra else "either"
    period = None if "--period" not in extra else tuple(float(v) for v in (extra[-1] + ",1,1").split(",")[:3]) \
        if "," in extra[-1] else float(extra[-1])
    per = {} if period is None else {"period": period}
    counts = E.reach_query_counts(p, q, rq, rp, rule=rule, **per)
    lists = E.reach_query_neighbors(p, q, rq, rp, rule=rule, **per)
    want = {".count": counts, ".offsets": lists[0], ".ids": lists[1], ".dist": lists[2]}
    pre = str(tmp_path / "reach")
    assert radius_app.main([fp, fq, "--reach", frq, frp, *extra, "-o", pre, "--device", "cpu"]) == 0
    for suf in SUFFIXES:
        assert _read(pre + suf) == want[suf].numpy().tobytes(), suf
    # chunks split along their prefix sums, and the squared values: byte-identical files
    largest = int(counts.max())
    pre2 = str(tmp_path / "split")
    assert radius_app.main([fp, fq, "--reach", frq, frp, *extra, "-o", pre2, "--device", "cpu", "--chunk", "64",
                            "--max-pairs", str(largest)]) == 0
    frq2, frp2, pre3 = str(tmp_path / "rq2.float"), str(tmp_path / "rp2.float"), str(tmp_path / "squared")
    io.write_array(frq2, rq * rq)
    io.write_array(frp2, rp * rp)
    assert radius_app.main([fp, fq, "--reach", frq2, frp2, "--squared", *extra, "-o", pre3, "--device", "cpu"]) == 0
    for suf in SUFFIXES:
        assert _read(pre2 + suf) == _read(pre + suf) == _read(pre3 + suf), suf
    pre4 = str(tmp_path / "counts")
    assert radius_app.main([fp, fq, "--reach", frq, frp, *extra, "-o", pre4, "--device", "cpu", "--counts-only",
                            "--stats", str(tmp_path / "s.json")]) == 0
    assert _read(pre4 + ".count") == _read(pre + ".count") and not os.path.exists(pre4 + ".ids")
    capsys.readouterr()
    # rcheck passes; under the other rule, and after one id is altered, it fails
    assert tools.main(["rcheck", fp, fq, pre, "--reach", frq, frp, *extra, "--samples", "400"]) == 0
    out = capsys.readouterr().out
    assert "sampled counts: 0 mismatches" in out and "sampled rows: 0 mismatches" in out
    assert tools.main(["rcheck", fp, fq, pre, "--reach", frq2, frp2, "--squared", *extra, "--samples", "400"]) == 0
    flipped = [a for a in extra if a not in ("--rule", "both")] + ([] if rule == "both" else ["--rule", "both"])
    assert tools.main(["rcheck", fp, fq, pre, "--reach", frq, frp, *flipped, "--samples", "400"]) == 1
    capsys.readouterr()
    first = int((counts > 3).nonzero()[0])
    ids = io.read_array(pre + ".ids", torch.int32)
    ids[int(lists[0][first])] += 1
    io.write_array(pre + ".ids", ids)
    assert tools.main(["rcheck", fp, fq, pre, "--reach", frq, frp, *extra, "--samples", "400"]) == 1
    assert "sampled rows: 1 mismatches" in capsys.readouterr().out


def test_cli_argument_errors(tmp_path, capsys):
    p, q = uniform(100, seed=13), uniform(10, seed=14)
    fp, fq = str(tmp_path / "p.float3"), str(tmp_path / "q.float3")
    frq, frp = str(tmp_path / "rq.float"), str(tmp_path / "rp.float")
    io.write_points(fp, p)
    io.write_points(fq, q)
    io.write_array(frq, torch.full((10,), 0.1))
    io.write_array(frp, torch.full((100,), 0.1))
    out = ["-o", str(tmp_path / "o"), "--device", "cpu"]
    for bad in (["--reach", frq], ["--reach", frq, frp, "-r", "0.1"], ["--reach", frq, frp, "--radii", frq],
                ["--reach", frq, frp, "--point-radii", frp], ["--reach", frq, frp, "--profile", "0.1"],
                ["--reach", frq, frp, "--rule", "neither"], ["-r", "0.1", "--rule", "both"],
                ["--radii", frq, "--rule", "either"]):
        with pytest.raises(SystemExit):
            radius_app.main([fp, fq, *bad, *out])
    capsys.readouterr()
    assert tools.main(["rcheck", fp, fq, str(tmp_path / "o"), "-r", "0.1", "--rule", "both"]) == 1
    # files of the wrong length, in either place: both lengths are named, nothing is written
    assert radius_app.main([fp, fq, "--reach", frp, frp, *out]) == 1
    err = capsys.readouterr().err
    assert "100 values" in err and "10 rows" in err
    assert radius_app.main([fp, fq, "--reach", frq, frq, *out]) == 1
    err = capsys.readouterr().err
    assert "10 values" in err and "100 rows" in err
    # a negative value, and one above half the period
    bad = torch.full((100,), 0.1)
    bad[2] = -1.0
    fbad = str(tmp_path / "bad.float")
    io.write_array(fbad, bad)
    assert radius_app.main([fp, fq, "--reach", frq, fbad, *out]) == 1
    bad[2] = 0.6
    io.write_array(fbad, bad)
    assert radius_app.main([fp, fq, "--reach", frq, fbad, "--period", "1", *out]) == 1
    assert "period" in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "o.count"))
    assert radius_app.main([fp, fq, "--reach", frq, fbad, *out]) == 0
    # the combinations that were refused stay refused, with their messages
    assert radius_app.main([fp, fq, "--point-radii", frp, "--period", "1", *out]) == 1
    assert "--period is not supported with --point-radii" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        radius_app.main([fp, fq, "--radii", frq, "--point-radii", frp, *out])
