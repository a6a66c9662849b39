"""Spec S25 on the CPU: the plain-Python restatement (score_spa_spec.py) against exact tails -- the convolution of two
binomials for an intercept-only null, the enumeration of all 2^16 outcomes next to a covariate --, its terms and its
root against mpmath at 50 digits, and the laws of the specification: the point mass of a perfectly predictive gene,
the side beyond the support, the cutoff, a gene and its complement, and no fallback on the problems the device is
held to (score_spa_cases.py)."""
import math

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


@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_no_fallback_on_the_problems_the_device_is_held_to(name):
    genes, values, cov = sc.problem(name)
    host = score_host(values, cov, "logistic")
    assert host["skipped"] == [None, "one_class", None]
    score = sc.s24(host, genes)
    spa_rows = np.concatenate([host["mu"][:, None, :], host["design"]], axis=1)
    assert spa_rows.shape == (sc.T, sc.SHAPES[name][2] + 2, sc.SHAPES[name][0])
    assert not spa_rows.transpose(0, 2, 1)[~host["valid"]].any()          # zero outside the valid sets
    every = sc.restate(spa_rows, host["rows"][:, 1], host["valid"], host["chol"], genes, score, sp.MIN_CUTOFF)
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
    if sc.RARE[N] < 0.1:                                                   # 5 % positives, rare genes, real statistics
        n, pos = int(host["n"][2]), np.nansum(values[2])
        assert 0.04 <= pos / n <= 0.07
        for g in range(3):
            m = int(genes[g][host["valid"][2]].sum())
            assert m <= 0.07 * n and score["stat"][2, g] > 30 and every[2][g]["p"] > 1e3 * score["p"][2, g]


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
