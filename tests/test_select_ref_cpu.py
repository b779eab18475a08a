"""The host oracle (K.kth_cpu, which every GPU test trusts) pinned to two references that
share nothing with it (select_ref.py), on the inputs that drive the select kernels'
recovery branches (test_gpu_select_paths.py). No GPU."""
import math

import numpy as np
import pytest
import torch

import select_ref as R
from mpi_cuda_largescaleknn_amd.ops import kernels as K


def _queries(c):
    p, q = R.case_input(c.name)
    rows = R.sample_rows(c)
    return p, (q if q is not None else p)[rows].contiguous()


def _cutoffs(c):
    """No cutoff; the `uniform` case also with the cutoffs the GPU test uses: the true k-th
    d² of one row (the median: half the rows lie below it, that row exactly on it), one
    float above it and one float below it."""
    if c.name != "uniform":
        return [math.inf]
    return [math.inf, *R.uniform_cutoffs(c.k)]


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_oracle_against_plain_references(c):
    p, q = _queries(c)
    assert q.shape[0] <= 2048
    for cut2 in _cutoffs(c):
        brute = K.kth_cpu(p, q, c.k, cut2, "brute")
        tree = K.kth_cpu(p, q, c.k, cut2, "kdtree")
        assert torch.equal(brute.view(torch.int32), tree.view(torch.int32)), "brute and kdtree differ"
        v = K.finalize_distances(brute).numpy()
        assert not np.isnan(v).any()
        ok = R.kth_bracket(p, q, v, c.k, cut2)
        assert ok.all(), f"{int((~ok).sum())} rows outside the float64 bracket (cut2={cut2})"
        plain, und, ties = R.kth_plain(p, q, c.k, cut2)
        # a condition on the input: the reference alone decides at least 99 % of the rows
        assert und.mean() <= 0.01, f"{int(und.sum())} of {und.size} rows undecided"
        same = plain.view(np.int32) == v.view(np.int32)
        assert same[~und].all(), f"{int((~same[~und]).sum())} decided rows differ from kth_plain"
        # the bracket is not vacuous: where the k-th value is untied the two counts differ by
        # exactly that one point (for at least 90 % of such rows)
        single = (ties == 1) & np.isfinite(v)
        if single.any():
            lo, hi = R.bracket_counts(p, q[torch.from_numpy(single)], v[single])
            frac = float((hi - lo == 1).mean())
            assert frac >= 0.9, f"bracket counts differ by the multiplicity on {frac:.3f} of {int(single.sum())} rows"
        # tied rows: the counts differ by at least the multiplicity (the ties lie inside)
        tied = (ties > 1) & np.isfinite(v)
        if tied.any():
            lo, hi = R.bracket_counts(p, q[torch.from_numpy(tied)], v[tied])
            assert (hi - lo >= ties[tied]).all()


def test_bracket_rejects_wrong_answers():
    """The bracket bites: the neighbouring ranks' distances, NaN and a wrong inf all fail."""
    c = next(x for x in R.CASES if x.name == "uniform")  # 20 000 points, k = 16
    p, q = _queries(c)
    q = q[:256].contiguous()
    for dk in (-1, 1):
        v = K.finalize_distances(K.kth_cpu(p, q, c.k + dk, math.inf, "brute")).numpy()
        assert not R.kth_bracket(p, q, v, c.k).any()
    assert not R.kth_bracket(p, q, np.full(256, np.nan, dtype=np.float32), c.k).any()
    assert not R.kth_bracket(p, q, np.full(256, np.inf, dtype=np.float32), c.k).any()
    assert R.kth_bracket(p[:10], q, np.full(256, np.inf, dtype=np.float32), c.k).all()


def test_rounding_tie_detection():
    """Flagged: exactly the float64 sums next to a float32 midpoint, and only inexact ones."""
    one = np.float64(1.0)
    ulp = np.float64(2.0 ** -23)
    s = np.array([one + 0.5 * ulp, one + 0.5 * ulp + 2.0 ** -52, one + 0.25 * ulp, one, one - 0.25 * ulp,
                  one - 0.25 * ulp + 2.0 ** -53, 0.0])
    _, tie = R._tie_f32(s)
    assert tie.tolist() == [True, True, False, False, True, True, False]
    # 1 + ulp/2 as an exact sum: round-half-even once, decided; with a lost 2^-60: flagged
    r, tie = R._round_f32(np.array([0.5 * ulp, 0.5 * ulp + 2.0 ** -60]), np.array([one, one]))
    assert tie.tolist() == [False, True] and r[0] == np.float32(1.0)


def test_status_bits_match_the_sources():
    for kern in ("rows", "grid"):
        assert R.parse_status_enum(kern) == R.status_bits[kern]
