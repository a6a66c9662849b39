"""Spec S25 on the CPU: the plain-Python restatement (score_spa_spec.py) against exact tails -- the convolution of two
binomials for an intercept-only null, the enumeration of all 2^16 outcomes next to a covariate --, its terms and its
root against mpmath at 50 digits, and the laws of the specification: the point mass of a perfectly predictive gene,
the side beyond the support, the cutoff, a gene and its complement, and no fallback on the problems the device is
held to (score_spa_cases.py)."""
import math
import os

import mpmath
import numpy as np
import pytest
from scipy.stats import binom

import score_spa_cases as sc
import score_spa_spec as sp
from scoary_amd.engine import score_host


def _one(values, cov, gene, cutoff=sp.MIN_CUTOFF):
    """(restatement's result, S24's outputs, items) of one trait and one gene through score_host."""
    host = score_host(np.asarray(values, dtype=np.float64)[None, :], cov, "logistic")
    assert host["skipped"] == [None]
    genes = np.asarray(gene, dtype=np.uint8)[None, :]
    score = sc.s24(host, genes)
    spa_rows = np.concatenate([host["mu"][:, None, :], host["design"]], axis=1)
    res = sc.restate(spa_rows, host["rows"][:, 1], host["valid"], host["chol"], genes, score, cutoff)[0][0]
    items = sp.projected(genes[0].tolist(), [r.tolist() for r in spa_rows[0]], host["rows"][0, 1].tolist(),
                         host["valid"][0].astype(int).tolist(), host["chol"][0].tolist(), score["b"][0, 0].tolist())
    return res, {k: v[0, 0] for k, v in score.items()}, items, host


def _table(n, m, k, a):
    """n isolates, the first k positive; m carriers, a of them positive."""
    y = np.zeros(n)
    y[:k] = 1
    g = np.zeros(n)
    g[:a] = 1
    g[k:k + m - a] = 1
    return y, g


# n, carriers m, positives k, positive carriers a
TABLES = [(2000, 10, 100, 4), (2000, 10, 100, 6), (2000, 30, 100, 8), (2000, 200, 100, 25), (500, 8, 25, 4)]


@pytest.mark.parametrize("n,m,k,a", TABLES)
def test_exact_tails_of_the_intercept_only_null(n, m, k, a):
    """S = (1 - m/n) A - (m/n) B with A ~ Bin(m, k/n) over the carriers and B ~ Bin(n - m, k/n) over the others: the
    exact two-sided tail is a sum over the lattice.  The saddlepoint p is within a factor 1.3 of it where Score_p is
    more than ten times too small.  Measured, saddlepoint / exact and exact / Score_p: 0.790 and 1.2e3; 0.800 and
    7.3e8; 1.000 and 7.5e2; 0.942 and 17; 0.901 and 2.8e4."""
    y, g = _table(n, m, k, a)
    res, score, _items, _host = _one(y, None, g, cutoff=sp.CUTOFF)
    assert res["status"] == 1
    mu = k / n
    A, B = np.arange(m + 1)[:, None], np.arange(n - m + 1)[None, :]
    S = (1.0 - m / n) * A - (m / n) * B
    pmf = binom.pmf(A, m, mu) * binom.pmf(B, n - m, mu)
    assert abs(score["U"] - ((1.0 - m / n) * a - (m / n) * (k - a))) <= 1e-12 * abs(score["U"])
    exact = float(pmf[np.abs(S) >= abs(score["U"]) * (1.0 - 1e-12)].sum())
    print("saddlepoint / exact %.4g, exact / Score_p %.4g" % (res["p"] / exact, exact / score["p"]))
    assert exact / 1.3 <= res["p"] <= exact * 1.3
    assert score["p"] * 10.0 < exact


ENUM_SEEDS = (2, 3, 4, 5, 7, 11, 12)


def test_full_enumeration_next_to_a_covariate():
    """n = 16 isolates, one covariate, genes of m = 3 carriers: the exact tail of S under the fitted null model is the
    sum over all 2^16 outcomes.  Over the 14 cases of these seeds with an exact p below 0.02 the median of
    |log(SPA_p / exact)| is 0.070, that of |log(Score_p / exact)| 0.471."""
    n, m = 16, 3
    Y = ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(np.float64)
    spa_err, score_err = [], []
    for seed in ENUM_SEEDS:
        rng = np.random.default_rng(seed)
        x = rng.standard_normal(n)
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(0.8 * x - 0.3)))).astype(np.float64)
        host = score_host(y[None, :], x[None, :], "logistic")
        assert host["skipped"] == [None]
        genes = np.zeros((30, n), dtype=np.uint8)
        for g in range(30):
            genes[g, rng.permutation(n)[:m]] = 1
        score = sc.s24(host, genes)
        spa_rows = np.concatenate([host["mu"][:, None, :], host["design"]], axis=1)
        every = sc.restate(spa_rows, host["rows"][:, 1], host["valid"], host["chol"], genes, score, sp.MIN_CUTOFF)[0]
        mu = host["mu"][0]
        prob = np.exp(Y @ np.log(mu) + (1.0 - Y) @ np.log1p(-mu))
        assert abs(prob.sum() - 1.0) < 1e-12
        for g in range(30):
            if not score["testable"][0, g]:
                continue
            items = sp.projected(genes[g].tolist(), [r.tolist() for r in spa_rows[0]], host["rows"][0, 1].tolist(),
                                 [1] * n, host["chol"][0].tolist(), score["b"][0, g].tolist())
            S = (Y - mu) @ np.array([it[0] for it in items])
            exact = float(prob[np.abs(S) >= abs(score["U"][0, g]) * (1.0 - 1e-12)].sum())
            if exact < 0.02:
                assert every[g]["status"] == 1
                spa_err.append(abs(math.log(every[g]["p"] / exact)))
                score_err.append(abs(math.log(score["p"][0, g] / exact)))
    print("cases %d, medians %.4g and %.4g" % (len(spa_err), np.median(spa_err), np.median(score_err)))
    assert len(spa_err) >= 10
    assert np.median(spa_err) < np.median(score_err)


def _mp_cgf(items, t):
    """(K, K', K'') at 50 digits, in the textbook form: K = sum log(1 - mu + mu e^{t g}) - t g mu."""
    with mpmath.workdps(50):
        t = mpmath.mpf(t)
        k0 = k1 = k2 = mpmath.mpf(0)
        for gt, mu, _w in items:
            gt, mu = mpmath.mpf(gt), mpmath.mpf(mu)
            e = mpmath.exp(t * gt)
            d = 1 - mu + mu * e
            k0 += mpmath.log(d) - t * gt * mu
            k1 += gt * mu * e / d - gt * mu
            k2 += gt * gt * mu * (1 - mu) * e / (d * d)
        return k0, k1, k2


def _mp_problems():
    y, g = _table(500, 8, 25, 4)
    yield _one(y, None, g)
    genes, values, cov = sc.problem("n65")
    for gene in (genes[0], genes[7], genes[-3]):
        keep = ~np.isnan(values[0])
        yield _one(values[0][keep], cov[:, keep], gene[keep])


def test_terms_and_root_against_mpmath():
    """K, K', K'' within 1e-13 relative of 50 digits at the roots, at half and at twice the roots, on both sides;
    K' - x changes sign between t^ (1 - 1e-10) and t^ (1 + 1e-10); K''(0) within 1e-14 relative of S24's Vg.  (Far
    below a root the two parts of a term of K, log1p(mu e) and a mu, cancel: of the order a^2 is left of two numbers
    of the order a, a relative error of about 2e-16 / |a|, which no statistic at or above the least cutoff meets:
    1.9e-13 at a hundredth of a root.)"""
    checked = 0
    for res, score, items, _host in _mp_problems():
        assert res["status"] == 1
        _k, _k1, k2 = sp.cgf(items, 0.0)
        assert _k == 0.0 and _k1 == 0.0
        assert abs(k2 - score["Vg"]) <= 1e-14 * score["Vg"], (k2, score["Vg"])
        for side, x in ((0, abs(score["U"])), (1, -abs(score["U"]))):
            t_hat = res["t"][side]
            assert math.isfinite(t_hat) and (t_hat > 0) == (x > 0)
            for t in (t_hat, 0.5 * t_hat, 2.0 * t_hat):
                got = sp.cgf(items, t)
                want = _mp_cgf(items, t)
                for name, a, b in zip(("K", "K'", "K''"), got, want):
                    assert abs(a - b) <= 1e-13 * abs(b), (name, t, a, float(b))
                checked += 1
            below = _mp_cgf(items, t_hat * (1.0 - 1e-10))[1] - x
            above = _mp_cgf(items, t_hat * (1.0 + 1e-10))[1] - x
            assert below * above < 0, (t_hat, float(below), float(above))
    assert checked == 24


def test_point_mass_of_a_perfectly_predictive_gene_and_the_side_beyond_the_support():
    """One covariate, 12 isolates, gene = trait: U is the upper end of the support, the upper tail is P(S = s_hi) by
    the enumeration of all outcomes under the fitted model, and -|U| lies beyond the lower end, where the enumeration
    finds nothing and S25 gives 0."""
    n = 12
    x = np.random.default_rng(5).standard_normal(n)
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    res, score, items, host = _one(y, x[None, :], y)
    lo, hi = sp.support(items)
    assert abs(score["U"] - hi) <= 1e-12 * hi and -abs(score["U"]) < lo * (1.0 + sp.EDGE)
    assert res["status"] == 1 and res["t"] == [math.inf, -math.inf] and res["z"] == [0.0, 0.0]
    Y = ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(np.float64)
    mu = host["mu"][0]
    prob = np.exp(Y @ np.log(mu) + (1.0 - Y) @ np.log1p(-mu))
    S = (Y - mu) @ np.array([it[0] for it in items])
    at_end = float(prob[S >= hi * (1.0 - 1e-12)].sum())
    assert at_end == pytest.approx(float(np.prod(np.where(y == 1, mu, 1.0 - mu))), rel=1e-12)
    assert abs(res["p"] - at_end) <= 1e-12 * at_end
    assert float(prob[S <= -abs(score["U"]) * (1.0 - 1e-12)].sum()) == 0.0
    assert sp.side(items, -abs(score["U"]), lo, False, score["Vg"]) == (0.0, -math.inf, 0.0)


def test_below_the_cutoff_the_p_is_score_p_bit_for_bit():
    genes, values, cov = sc.problem("n130")
    keep = ~np.isnan(values[0])
    seen = set()
    for gene in genes[:12]:
        for cutoff in (sp.MIN_CUTOFF, sp.CUTOFF, 50.0):
            res, score, _items, _host = _one(values[0][keep], cov[:, keep], gene[keep], cutoff=cutoff)
            below = score["stat"] < cutoff * cutoff
            seen.add((cutoff, bool(below)))
            assert (res["status"] == 0) == below
            if below:
                assert np.float64(res["p"]).view(np.uint64) == np.float64(score["p"]).view(np.uint64)
                assert res["z"] == [0.0, 0.0] and res["t"] == [0.0, 0.0]
    assert {(sp.CUTOFF, True), (sp.MIN_CUTOFF, False), (50.0, True)} <= seen
    for bad in (0.0999, 0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            sp.spa([0], [[0.5], [1.0]], [0.25], [1], [1.0], 0.0, [0.0], 0.0, 0.0, 1.0, cutoff=bad)


def test_a_gene_and_its_complement_get_the_same_p():
    """The complement's projection is the gene's with the other sign (the column of ones is in the design), so U
    changes sign and the two tails change places."""
    genes, values, cov = sc.problem("n65")
    keep = ~np.isnan(values[2]) & ~np.isnan(cov).any(axis=0)
    done = 0
    for gene in genes[:10]:
        a, sa, _i, _h = _one(values[2][keep], cov[:, keep], gene[keep])
        b, sb, _i, _h = _one(values[2][keep], cov[:, keep], 1 - gene[keep])
        if a["status"] != 1:
            continue
        assert b["status"] == 1 and abs(sa["U"] + sb["U"]) <= 1e-9 * abs(sa["U"])
        assert abs(a["p"] - b["p"]) <= 1e-9 * a["p"]
        done += 1
    assert done >= 5


_PROBLEMS = {}


def _problem(name):
    """A problem of score_spa_cases on the host, once: (what restate takes before the score, S24's outputs, the
    listed pairs, the restatement at the least cutoff -- [T][G], or the dict of the listed pairs --, host, values).
    name: a shape, "fallback", "ends" (ends_problem as it is), "ends moved" (its fabricated ends), "wide"."""
    if name in _PROBLEMS:
        return _PROBLEMS[name]
    subset = None
    if name == "wide":
        genes, values, cov = sc.wide_problem()
        subset = sc.wide_candidates()
    elif name.startswith("ends"):
        genes, values, cov = sc.ends_problem()
    else:
        genes, values, cov = sc.fallback_problem() if name == "fallback" else sc.problem(name)
    host = score_host(values, cov, "logistic")
    spa_rows = np.concatenate([host["mu"][:, None, :], host["design"]], axis=1)
    P = (spa_rows, host["rows"][:, 1], host["valid"], host["chol"], genes)
    score = sc.s24(host, genes, subset)
    listed = None
    if name in sc.SUBSET:
        listed = list(sc.LISTED[name])
    elif name == "wide":
        listed = sc.wide_listed(score["stat"])
    elif name == "ends moved":
        U, _what = sc.ends_moves(*P, score)
        listed = list(U)
        score = sc.fabricate(score, listed, U)
    if listed is None:
        every = sc.restate(*P, score, sp.MIN_CUTOFF)
        listed = [(t, g) for t in range(len(every)) for g in range(len(genes)) if every[t][g]["status"]]
    else:
        every = sc.restate(*P, sc.fabricate(score, listed), sp.MIN_CUTOFF, pairs=listed)
    _PROBLEMS[name] = (P, score, listed, every, host, values)
    return _PROBLEMS[name]


# the shapes whose trait 2 is itself a point mass as gene 3 (more covariates move that gene off the end of the support)
OWN_GENE_AT_THE_END = ("n64", "n130", "n600", "n97", "n113", "n150")


@pytest.mark.parametrize("name", list(sc.EVERY_PAIR))
def test_no_fallback_on_the_problems_the_device_is_held_to(name):
    P, score, _listed, every, host, values = _problem(name)
    spa_rows, genes = P[0], P[4]
    assert host["skipped"] == [None, "one_class", None]
    assert spa_rows.shape == (sc.T, sc.SHAPES[name][2] + 2, sc.SHAPES[name][0])
    assert not spa_rows.transpose(0, 2, 1)[~host["valid"]].any()          # zero outside the valid sets
    status = np.array([[r["status"] for r in row] for row in every])
    assert not (status == 2).any()
    assert np.array_equal(status == 1, score["testable"] & (score["stat"] >= sp.MIN_CUTOFF ** 2))
    assert not status[1].any()                                             # the skipped trait
    G, N = len(genes), sc.SHAPES[name][0]
    assert (score["stat"][0] >= sp.CUTOFF ** 2).sum() >= 1                 # every shape reaches the search by default
    if G >= 70:
        assert every[0][G - 4]["t"][0] == math.inf                         # the perfectly predictive gene
        assert status[0, G - 5] == 0 and not score["testable"][0, G - 5]   # the gene in the span of the covariates
        assert (score["stat"][2] >= sp.CUTOFF ** 2).sum() >= 5 and (status == 0).sum() > sc.T
        if sc.SHAPES[name][2] <= 2:                                        # the rare trait's own (eight covariates
            assert every[2][3]["t"][0] == math.inf                         # move that gene off the end of the support)
        assert (every[2][3]["t"][0] == math.inf) == (name in OWN_GENE_AT_THE_END)
    if sc.RARE[N] < 0.1:                                                   # 5 % positives, rare genes, real statistics
        n, pos = int(host["n"][2]), np.nansum(values[2])
        assert 0.04 <= pos / n <= 0.07
        for g in range(3):
            m = int(genes[g][host["valid"][2]].sum())
            assert m <= 0.07 * n and score["stat"][2, g] > 30 and every[2][g]["p"] > 1e3 * score["p"][2, g]


def test_every_instance_has_a_shape():
    """q = 1 .. 9: every instance of the search and of the sums runs in some shape that is restated over every pair."""
    assert {sc.SHAPES[name][2] + 1 for name in sc.EVERY_PAIR} == set(range(1, 10))
    new = [sc.SHAPES[name] for name in ("n97", "n113", "n128", "n150", "n177", "n199")]
    assert all(96 <= N <= 200 and G == 70 for N, G, _c in new) and sum(N % 32 != 0 for N, _G, _c in new) >= 3
    assert len({N for N, _G, _c in sc.SHAPES.values()}) == len(sc.SHAPES) == len(sc.RARE) == len(sc.SEEDS)


@pytest.mark.parametrize("name", list(sc.SUBSET) + ["wide"])
def test_the_listed_pairs_of_the_long_and_wide_problems_have_status_1(name):
    """n4099, n65536 and wide_problem are held through listed pairs: each testable, none falling back; n4099's
    include the rare genes, a point mass on each of two traits and a side beyond the support."""
    P, score, listed, every, host, _values = _problem(name)
    assert len(listed) == len(set(listed)) == {"n4099": 12, "n65536": 2, "wide": 64}[name]
    assert all(score["testable"][pair] and every[pair]["status"] == 1 for pair in listed)
    if name == "n4099":
        G = len(P[4])
        assert host["skipped"] == [None, "one_class", None] and {(2, 0), (2, 1), (2, 2), (0, G - 4)} <= set(listed)
        assert every[0, G - 4]["t"] == [math.inf, -math.inf] and every[2, 3]["t"][0] == math.inf
        assert all(score["stat"][2, g] > 30 and every[2, g]["p"] > 1e3 * score["p"][2, g] for g in range(3))
    if name == "n65536":
        assert host["skipped"] == [None, "one_class", None] and P[0].shape[2] == 65536
    if name == "wide":
        N, G, Tn = sc.WIDE
        at = sorted(t * G + g for t, g in listed)
        assert Tn * G > 2048 * 256 and at[0] == 0 and at[-1] == Tn * G - 1 and host["skipped"] == [None] * Tn
        assert {524286, 524287, 524288, 524289} <= set(at) and set(range(262144, 262154)) <= set(at)


def test_the_ends_of_the_support_on_both_sides():
    """ends_problem: the perfectly anti-predictive gene has U < 0, the point mass below and nothing above; the moved
    pairs are beyond the support (tail 0), at the point mass from either side of the end (its tail, an infinite t^),
    and at roots a hundredth and a ten-thousandth of the support from the end, of which at least two per side and
    distance end within 80 evaluations with status 1 -- on side 0 and on side 1."""
    P, score, _listed, every, _host, _values = _problem("ends")
    G = len(P[4])
    anti = every[0][G - 1]
    items = sc.items_of(*P, score, 0, G - 1)
    lo, _hi = sp.support(items)
    assert score["U"][0, G - 1] < 0.0 and abs(score["U"][0, G - 1] - lo) <= 1e-12 * abs(lo)
    assert anti["status"] == 1 and anti["t"] == [math.inf, -math.inf] and anti["tails"][0] == 0.0
    assert abs(anti["p"] - sp.point_mass(items, False)) <= 1e-10 * anti["p"] and anti["p"] > 0.0
    assert abs(anti["p"] - every[0][G - 5]["p"]) <= 1e-9 * anti["p"]      # trait 0 itself: the same mass, above
    _P, fab, listed, moved, _host, _values = _problem("ends moved")
    _U, what = sc.ends_moves(*P, score)
    assert list(what) == listed
    kept = {}
    for pair, (side, kind, v) in what.items():
        r = moved[pair]
        assert r["status"] == 1, (pair, side, kind, v)
        kept[side, kind, v] = kept.get((side, kind, v), 0) + 1
        if kind == "k":
            assert math.isinf(r["t"][side]) and r["z"][side] == 0.0
            assert (r["tails"][side] == 0.0) if v > 1.0 else (0.0 < r["tails"][side] < 1e-30), (pair, r)
        else:
            assert math.isfinite(r["t"][side]) and abs(r["t"][side]) > 10.0
    assert kept == dict([((side, "k", k), 1) for side in (0, 1) for k in sc.ENDS_K] +
                        [((side, "delta", d), kept.get((side, "delta", d))) for side in (0, 1) for d in sc.ENDS_DELTA])
    assert all(kept[side, "delta", d] >= 2 for side in (0, 1) for d in sc.ENDS_DELTA)


CENSUS = list(sc.EVERY_PAIR) + ["fallback"] + list(sc.SUBSET) + ["ends", "ends moved", "wide"]
CENSUS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "score_spa_tests.txt")
CENSUS_ROOM = 80


def _census():
    """{problem: [(t, g, side, evaluations, rules, status, root)]}: score_spa_cases.device_search over every listed
    side of every problem the device is held to, at the least cutoff."""
    out = {}
    for name in CENSUS:
        P, score, listed, every, _host, _values = _problem(name)
        out[name] = sc.census(*P, score, listed, every)
    return out


def census_text(census):
    """The text of profiles/score_spa_tests.txt below its head: per problem the searched sides by evaluations."""
    edges = (0, 10, 20, 30, 40, 50, 60, 80, sc.DEVICE_MAX_EVALS + 1)
    lines = ["%-11s %5s  " % ("problem", "sides") + " ".join("%7s" % ("%d-%d" % (a, b - 1)) for a, b in
                                                              zip(edges, edges[1:])) + "   max  at the cap"]
    for name, rows in census.items():
        evals = [r[3] for r in rows]
        hist = [sum(a <= e < b for e in evals) for a, b in zip(edges, edges[1:])]
        lines.append("%-11s %5d  " % (name, len(rows)) + " ".join("%7d" % h for h in hist) +
                     " %5d  %d" % (max(evals), sum(r[6] is None for r in rows)))
    for rule in sc.RULES:
        lines.append("rule %-18s sides %d" % (rule + ":", sum(rule in r[4] for rows in census.values() for r in rows)))
    return "\n".join(lines) + "\n"


def test_search_census():
    """The device's search rule (score_spa_cases.device_search) over every searched side of every problem the device
    is held to: each of its five rules is used; no side of a pair with the restatement's status 1 stops at the cap of
    100 evaluations, or takes more than 80 -- a condition on the problems, which leaves 20 evaluations to the device's
    own rounding (its sums are not math.fsum's; how many evaluations it takes has not been measured).  The side that
    takes 64, above the cap of 60 that S25 had: n600, trait 0, the perfectly predictive gene, the lower side.
    Running this file as a program from the repository root writes the census to profiles/score_spa_tests.txt."""
    census = _census()
    used = set().union(*(r[4] for rows in census.values() for r in rows))
    assert used == set(sc.RULES)
    for name, rows in census.items():
        for t, g, side, evals, _rules, status, root in rows:
            if status == 1:
                assert root is not None and evals <= CENSUS_ROOM, (name, t, g, side, evals)
    G = sc.SHAPES["n600"][1]
    slow = [r for r in census["n600"] if r[:3] == (0, G - 4, 1)]
    assert len(slow) == 1 and slow[0][3] > 60 and slow[0][5] == 1       # the side the cap of 60 sent to Score_p
    assert max(r[3] for rows in census.values() for r in rows if r[5] == 1) == max(r[3] for r in census["n600"])
    with open(CENSUS_FILE) as f:
        text = f.read()
    assert all(("\n%-11s " % name) in text for name in CENSUS) and all(rule in text for rule in sc.RULES)


def test_the_fallback_problem_falls_back_where_it_is_meant_to():
    """n130 with the 5 % trait's values kept at the carriers of the one- and two-carrier genes: those two pairs, with
    no positive carrier and a statistic of 0.08, have a lower z of the upper side's sign: status 2, Score_p."""
    genes, values, cov = sc.fallback_problem()
    host = score_host(values, cov, "logistic")
    score = sc.s24(host, genes)
    spa_rows = np.concatenate([host["mu"][:, None, :], host["design"]], axis=1)
    every = sc.restate(spa_rows, host["rows"][:, 1], host["valid"], host["chol"], genes, score, sp.MIN_CUTOFF)
    G = len(genes)
    fell = [(t, g) for t in range(sc.T) for g in range(G) if every[t][g]["status"] == 2]
    assert fell == [(2, G - 2), (2, G - 1)]
    for t, g in fell:
        assert every[t][g]["p"] == score["p"][t, g] and 0.05 < score["stat"][t, g] < 0.1
        assert not (genes[g] * np.nan_to_num(values[t]))[host["valid"][t]].any()
    assert not any(r["status"] == 2 for row in sc.at_cutoff(every, score, sp.CUTOFF) for r in row)


if __name__ == "__main__":
    HEAD = """score_spa_tests: the census of the device's search rule over the problems of the device tests
(tests/test_score_spa_spec.py::test_search_census; written by `PYTHONPATH=. python tests/test_score_spa_spec.py`).

score_spa_cases.device_search is S25's "The search (device)" in plain Python with the sums by math.fsum.  It was run
over every searched side (not beyond the support, not a point mass) of every pair that the device tests list, at the
least cutoff 0.1.  Columns: sides by evaluations of K', K''; the most; sides that stop at the cap of 100.
A CPU census: deterministic, no GPU.  NOT MEASURED: how many evaluations the device itself takes.  Its sums round
differently from math.fsum, and near the rounding floor of K' that changes which rule a step takes.  The tests hold
the problems to at most 80 evaluations where the restatement has status 1; the 20 up to the cap are the room left for
that difference, and nobody has measured how much of it is used.

The slowest side: n600, trait 0, gene G - 4 (the perfectly predictive gene, stat 561, |U| at 0.999996 of the lower
end of the support), the lower side: %d evaluations -- above the cap of 60 that S25 had until this census, under which
the pair could only get Score_p.  Its trace: 15 Newton steps that creep up, one 4t step to where K'' is about 0, 23
midpoints, then Newton and midpoint in turn at the rounding floor of K'.  About 30 %% of the sides of n64 and n600
take 30 to 49 evaluations in that slow mode (midpoints while the upper end of the bracket sits where K'' is about 0).

Mutation check of the device tests (tests/test_gpu_score_spa.py on one MI355X, libraries built from mutated copies
of scoary_score_spa.hip outside the tree; which tests go red):
  isolates skipped by a zero weight instead of the validity bit   test_invalid_isolates_are_skipped_by_their_bit
                                                                   alone, both shapes (every older test passes)
  sums indexed by o %% count in k_spa_finish                        test_select_strides_and_the_list_is_free and 27 more
  log(m) and log1p(-m) swapped in the point-mass walk              test_the_ends_of_the_support_on_both_sides, and
                                                                   the restated shapes
  the row step xi += N dropped at j = 4                            n128, n150, n177, n199 (q = 5 .. 8) and n65
  the cap back at 60 in device_search (CPU)                        test_search_census: n600, trait 0, gene 66, side 1
(The mu[i] load moved in front of the validity test was not built: its value is unused on the path that returns
false, so the compiler is free to drop it; the mutant above is the form of that mistake that survives a compiler.)

"""
    census = _census()
    G = sc.SHAPES["n600"][1]
    slow = [r[3] for r in census["n600"] if r[:3] == (0, G - 4, 1)][0]
    with open(CENSUS_FILE, "w") as f:
        f.write(HEAD % slow + census_text(census))
    print(open(CENSUS_FILE).read())
