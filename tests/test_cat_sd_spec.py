"""Spec S23 without a GPU: the consequences DESIGN.md states for the step-down maxT of the categorical tests, checked on
the plain-numpy restatement (cat_sd_spec.py) over random small problems of both tests, and the planted driver on which
the step-down count is strictly below the single-step one.  The rows of the random problems are numpy shuffles -- over
the labelled isolates, or within the strata: the consequences hold for any rows that keep the margins --; the planted
driver runs under the project's own permutation law."""
import numpy as np
import pytest

import cat_sd_spec as sd
import cat_wy_spec as ws

PROBLEMS = 200


def _problem(i):
    """Random problem i: (genes [G, N], codes [N], strata [N], S, rows for the chi-square test, rows for gcmh).  K runs
    over 2 .. 8; every third problem has an empty class in the middle, every other one isolates without a label;
    strata of one and of two isolates come first; duplicated and complemented genes make tie groups, an absent and an
    ubiquitous gene are untestable."""
    rng = np.random.default_rng(2300 + i)
    K = 2 + i % 7
    N = int(rng.integers(max(6, K + 3), 30))
    G = 1 if i % 25 == 0 else int(rng.integers(3, 12))
    P = int(rng.integers(15, 40))
    codes = rng.integers(1, K + 1, N)
    codes[:K] = np.arange(1, K + 1)
    if i % 3 == 0 and K >= 3:
        codes[codes == 2] = 1                              # an empty class in the middle
    if i % 2 == 0:
        codes[rng.random(N) < 0.15] = 0                    # isolates without a label
    S = int(rng.integers(3, 6))
    strata = rng.integers(2, S, N)
    strata[0], strata[1], strata[2] = 0, 1, 1              # a stratum of one isolate and one of two
    strata[N - 1] = S - 1
    genes = (rng.random((G, N)) < rng.uniform(0.2, 0.8, (G, 1))).astype(np.int64)
    if G >= 6:
        genes[3] = genes[0]                                # a tie group of two equal genes ..
        genes[4] = 1 - genes[0]                            # .. and the complement, where every isolate has a label
        genes[1] = 0
        genes[2] = 1
    valid = np.flatnonzero(codes)
    chi_rows = np.tile(codes, (P, 1))
    gcmh_rows = np.tile(codes, (P, 1))
    for p in range(P):
        chi_rows[p, valid] = rng.permutation(codes[valid])
        for s in range(S):
            idx = valid[strata[valid] == s]
            gcmh_rows[p, idx] = rng.permutation(codes[idx])
    return genes, codes, strata, S, chi_rows, gcmh_rows


def _traits(i):
    genes, codes, strata, S, chi_rows, gcmh_rows = _problem(i)
    return genes, (("chi2", sd.chi2_trait(genes, codes, chi_rows)),
                   ("gcmh", sd.gcmh_trait(genes, codes, strata, S, gcmh_rows)))


def test_the_problems_cover_what_they_claim():
    seen = dict(K=set(), empty=0, missing=0, one=0, ties=0, untestable=0, g1=0)
    for i in range(PROBLEMS):
        genes, codes, strata, S, _c, _g = _problem(i)
        seen["K"].add(int(codes.max()))
        present = set(codes[codes > 0].tolist())
        seen["empty"] += any(k not in present for k in range(1, int(codes.max())))
        seen["missing"] += bool((codes == 0).any())
        sizes = np.bincount(strata, minlength=S)
        assert sizes[0] == 1 and sizes[1] == 2
        seen["g1"] += len(genes) == 1
        _genes, traits = _traits(i)
        for _name, tr in traits:
            thr = tr["thr"]
            seen["ties"] += len(set(thr[thr > 0].tolist())) < int((thr > 0).sum())
            seen["untestable"] += bool((thr == 0).any())
    assert seen["K"] == set(range(2, 9))
    assert min(seen[k] for k in ("empty", "missing", "ties", "untestable", "g1")) >= 8, seen


def test_the_consequences_over_random_problems():
    strict = {"chi2": 0, "gcmh": 0}
    for i in range(PROBLEMS):
        genes, traits = _traits(i)
        G = len(genes)
        for name, tr in traits:
            cells, thr, r = tr["cells"], tr["thr"], tr["r"]
            P = cells.shape[0]
            out = sd.stepdown(cells, thr)
            mx = ws.maxs(cells)
            r_fwer = ws.r_fwer(mx, thr)
            r_sd = out["r_sd"]
            # u[0] is S22's maximum, bit for bit
            assert np.array_equal(out["u"][0].view(np.int64), mx.view(np.int64)), (i, name)
            # r <= r_sd <= r_fwer
            assert (r <= r_sd).all() and (r_sd <= r_fwer).all(), (i, name)
            strict[name] += int((r_sd < r_fwer).sum())
            # equality on the tie group at rank 0, and with one gene
            top = thr == thr.max()
            assert np.array_equal(r_sd[top], r_fwer[top]), (i, name)
            if G == 1:
                assert np.array_equal(r_sd, r_fwer)
            # thr = 0 sorts last and counts every permutation, with no special case
            assert (r_sd[thr == 0] == P).all(), (i, name)
            assert (thr[tr["s_obs"] == 0] == 0).all()
            if name == "chi2":
                assert (thr[tr["ivm"] == 0] == 0).all()
            else:
                assert (thr[tr["df"] == 0] == 0).all()
            # the order inside a tie group does not matter: descending thr, ties by DESCENDING gene index
            other = np.asarray(sorted(range(G), key=lambda g: (-thr[g], -g)), dtype=np.int64)
            assert np.array_equal(sd.stepdown(cells, thr, order=other)["r_sd"], r_sd), (i, name)
            # nor does the order of the genes in the table
            perm = np.random.default_rng(i).permutation(G)
            moved = sd.stepdown(cells[:, perm], thr[perm])["r_sd"]
            assert np.array_equal(moved, r_sd[perm]), (i, name)
            # c adds over batches of permutations; the tail runs once, behind the last
            h = P // 2
            c2 = sd.stepdown(cells[:h], thr)["c"] + sd.stepdown(cells[h:], thr)["c"]
            assert np.array_equal(c2, out["c"]), (i, name)
            assert np.array_equal(sd.tail(c2, out["tt"], out["order"]), r_sd)
            # the adjusted p
            assert np.array_equal(sd.adjusted_p(r_sd, P), (r_sd + 1.0) / (P + 1.0))
    assert strict["chi2"] > 0 and strict["gcmh"] > 0       # (the step-down gains something somewhere)


def test_two_statistics_one_ulp_apart_that_round_to_one_thr_form_one_tie_group():
    # thr = s (1 - 1e-9) steps by a little less than one ulp where s steps by one, so once in about 1e9 steps two
    # neighbours round to one thr: in [2, 4) s = k 2^-51, and that happens where k c (c = 1 - fl(1 - 1e-9)) passes a
    # half-integer.  The place is computed in the rationals and confirmed in doubles.
    from fractions import Fraction
    c = 1 - Fraction(ws.ONE_MINUS_BAND)
    k = int((Fraction(5_000_000) + Fraction(1, 2)) / c)
    assert 2 ** 52 <= k - 3 and k + 4 < 2 ** 53
    found = None
    for d in range(-3, 4):
        s = float(Fraction(k + d, 2 ** 51))
        up = float(np.nextafter(s, np.inf))
        if ws.thr_of(s) == ws.thr_of(up):
            found = (s, up)
    assert found is not None
    thr = np.array([ws.thr_of(found[1]), ws.thr_of(found[0]), 1.0])
    cells = np.array([[0.0, thr[0], 0.0], [0.0, 0.0, 2.0], [0.0, 0.0, 0.0]])      # [P, G]
    out = sd.stepdown(cells, thr)
    assert thr[0] == thr[1] and out["order"].tolist() == [0, 1, 2]
    assert out["c"].tolist() == [1, 1, 1] and out["r_sd"].tolist() == [1, 1, 1]
    # the exceedance at the group's first gene alone: the second position's own count is 0, and it takes the first's
    cells2 = np.array([[thr[0], 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    out2 = sd.stepdown(cells2, np.array([thr[0], thr[1], 0.0]))
    assert out2["c"].tolist() == [1, 0, 3] and out2["r_sd"].tolist() == [1, 1, 3]


@pytest.mark.parametrize("test", ("chi2", "gcmh"))
def test_the_planted_driver_gains_from_the_step_down(test):
    genes, codes, _strata, tr, out, r_fwer = sd.planted_problem(test)
    assert genes.shape == (40, 60) and int(codes.max()) == 3 and tr["cells"].shape == (sd.PLANTED_P, 40)
    r_sd = out["r_sd"]
    assert out["order"][0] == 0 and r_fwer[0] == 0 and r_sd[0] == 0          # no permuted row reaches the driver
    assert (tr["r"] <= r_sd).all() and (r_sd <= r_fwer).all()
    assert int((r_sd < r_fwer).sum()) >= 1                                   # strictly below for at least one gene
    assert (sd.adjusted_p(r_sd, sd.PLANTED_P) <= sd.adjusted_p(r_fwer, sd.PLANTED_P)).all()
