"""Spec S16 without a GPU: the restatement (vanelteren_spec.py) against SciPy, its invariants, the law of the
shuffle within strata, and the engine's host ranking (engine.vanelteren_rows) against the restatement."""
import math

import numpy as np
import pytest

import ranksum_spec as rs
import vanelteren_spec as ve


def _trait(rng, N, S, ties=True, missing=0.1):
    x = np.round(rng.standard_normal(N), 1) if ties else rng.standard_normal(N)
    x[rng.random(N) < missing] = math.nan
    return [float(v) for v in x], [int(s) for s in rng.integers(0, S, N)]


def _genes(rng, G, N):
    return (rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))).astype(int)


def test_one_stratum_is_scipys_mannwhitneyu_without_continuity():
    """S = 1: p within 1e-12 relative of scipy.stats.mannwhitneyu(use_continuity=False, method="asymptotic")."""
    from scipy import stats
    rng = np.random.default_rng(16)
    N = 300
    x, _ = _trait(rng, N, 1)
    pl = ve.plan(x, [0] * N, 1)
    assert pl["w"] == [ve.MAX_SCORE // (pl["n"][0] + 1)]
    worst = 0.0
    for gene in _genes(rng, 50, N):
        D, ms = ve.statistic(gene, pl)
        ok, var, den, auc, p = ve.tail(D, ms, pl)
        a = [x[i] for i in range(N) if gene[i] and pl["valid"][i]]
        b = [x[i] for i in range(N) if not gene[i] and pl["valid"][i]]
        want = stats.mannwhitneyu(a, b, use_continuity=False, method="asymptotic")
        assert ok and den == pl["w"][0] * len(a) * len(b)
        worst = max(worst, abs(p - want.pvalue) / want.pvalue)
        assert auc == pytest.approx(want.statistic / (len(a) * len(b)), rel=1e-12)
    print("worst relative difference of p: %.3g" % worst)
    assert worst < 1e-12


def test_strata_are_a_direct_float_van_elteren():
    """S = 7: p within 1e-12 relative of the textbook statistic from scipy.stats.rankdata per stratum with the same
    integer weights: T = sum w_s (R_s - m_s (n_s + 1) / 2), Var = sum w_s^2 m_s (n_s - m_s) / 12 (n_s + 1 - tie)."""
    from scipy import stats
    rng = np.random.default_rng(17)
    N, S = 300, 7
    x, st = _trait(rng, N, S)
    pl = ve.plan(x, st, S)
    worst = 0.0
    for gene in _genes(rng, 50, N):
        D, ms = ve.statistic(gene, pl)
        ok, var, den, auc, p = ve.tail(D, ms, pl)
        stat, v = 0.0, 0.0
        for s in range(S):
            who = [i for i in range(N) if st[i] == s and pl["valid"][i]]
            n, w = len(who), ve.weight(len(who))
            if n < 2:
                continue
            ranks = stats.rankdata([x[i] for i in who])
            m = sum(int(gene[i]) for i in who)
            tau = np.unique([x[i] for i in who], return_counts=True)[1]
            stat += w * (sum(r for r, i in zip(ranks, who) if gene[i]) - m * (n + 1) / 2.0)
            v += w * w * m * (n - m) / 12.0 * (n + 1 - float(np.sum(tau ** 3 - tau)) / (n * (n - 1)))
        want = math.erfc(abs(stat) / math.sqrt(v) / math.sqrt(2.0))
        assert ok and 2 * stat == D
        worst = max(worst, abs(p - want) / want)
    print("worst relative difference of p: %.3g" % worst)
    assert worst < 1e-12


@pytest.mark.parametrize("sizes", ((16319, 1), (8160, 8160), (8160, 2, 1, 0, 5)))
def test_scores_sum_to_zero_per_stratum_and_fit_two_digits(sizes):
    """Strata of 16 319 (w = 1), 8 160 (w = 1, just above 8 159), 2, 1 and 0 valid isolates: the scores of every
    stratum sum to 0, |a| <= 16 319, and the hi digit of S15's split fits a signed byte."""
    rng = np.random.default_rng(sum(sizes))
    st = [s for s, k in enumerate(sizes) for _ in range(k)]
    x = [float(v) for v in rng.integers(0, 4000, len(st))]
    x[0], x[1] = -1.0, 5000.0                              # the extreme ranks of stratum 0, untied
    pl = ve.plan(x, st, len(sizes))
    assert pl["n"] == list(sizes)
    assert pl["w"] == [0 if k == 0 else max(1, 16319 // (k + 1)) for k in sizes]
    assert pl["w"][0] == 1 and ve.weight(8159) == 1 and ve.weight(8158) == 2 and ve.weight(1) == 8159
    for s in range(len(sizes)):
        assert sum(a for a, t in zip(pl["score"], st) if t == s) == 0
    assert max(abs(a) for a in pl["score"]) <= ve.MAX_SCORE
    assert (pl["score"][0], pl["score"][1]) == (-(sizes[0] - 1) * pl["w"][0], (sizes[0] - 1) * pl["w"][0])
    assert all(-128 <= rs.digits(a)[0] <= 127 for a in pl["score"])
    assert len(pl["L"]) == sum(sizes) and sorted(pl["L"]) == sorted(pl["score"])


def test_untestable_genes_have_d_zero_in_every_permuted_row():
    """No stratum with carriers and non-carriers among its valid isolates, or every such stratum fully tied:
    var <= 0, (auc 0.5, p 1), and D = 0 for the observed and for every permuted row."""
    nan = math.nan
    x = [1.0, 2.0, 3.0, nan, 7.0, 7.0, 7.0, 4.0, 0.5, 9.0, nan]
    st = [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3]                 # stratum 1 fully tied, stratum 3 without a value
    pl = ve.plan(x, st, 4)
    assert pl["n"] == [3, 3, 3, 0] and pl["c"][1] == 0.0 and pl["c"][3] == 0.0 and pl["w"][3] == 0
    genes = ([1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0],            # the whole of stratum 0
             [1, 1, 1, 0, 1, 0, 0, 1, 1, 1, 1],            # whole strata, and a split of the tied one
             [0] * 11, [1] * 11,
             [0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1])            # invalid isolates and the tied stratum only
    for gene in genes:
        D, ms = ve.statistic(gene, pl)
        assert ve.tail(D, ms, pl)[0] is False and ve.tail(D, ms, pl)[3:] == (0.5, 1.0) and D == 0
        for pi in range(40):
            assert ve.statistic(gene, pl, ve.perm_row(5, 0, pi, pl))[0] == 0
    D, ms = ve.statistic([1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], pl)
    assert ve.tail(D, ms, pl)[0] is True and D != 0


def test_permuted_rows_keep_every_stratums_scores_and_the_zeros():
    rng = np.random.default_rng(4)
    N, S = 120, 5
    x, st = _trait(rng, N, S, missing=0.2)
    st = [s if s != 3 else 2 for s in st]                  # stratum 3 is empty
    pl = ve.plan(x, st, S)
    moved = 0
    for pi in range(30):
        row = ve.perm_row(99, 2, pi, pl)
        assert all(row[i] == 0 for i in range(N) if not pl["valid"][i])
        for s in range(S):
            who = [i for i in range(N) if st[i] == s and pl["valid"][i]]
            assert sorted(row[i] for i in who) == sorted(pl["score"][i] for i in who)
        moved += row != pl["score"]
        assert row == ve.perm_row(99, 2, pi, pl) and row != ve.perm_row(99, 1, pi, pl)
    assert moved == 30


def test_one_stratum_rows_are_the_weight_times_s15s():
    rng = np.random.default_rng(6)
    N = 70
    x, _ = _trait(rng, N, 1)
    pl = ve.plan(x, [0] * N, 1)
    valid, rc, n, tiesum, _ = rs.ranks(x)
    assert pl["valid"] == valid and pl["score"] == [pl["w"][0] * r for r in rc] and ve.strata_bits(1) == 0
    for pi in (0, 1, 17):
        assert ve.perm_row(3, 1, pi, pl) == [pl["w"][0] * r for r in rs.perm_row(3, 1, pi, valid, rc)]
    assert [ve.strata_bits(S) for S in (2, 3, 4, 5, 1000, 1024)] == [1, 2, 2, 3, 10, 10]


def test_the_law_of_the_shuffle_within_strata_is_uniform():
    """Strata of 3 and 2 valid isolates with distinct values: the 3! 2! = 12 joint orders are equally likely.
    P = 24 000 permutations at seed 1, 2000 expected per order; chi-square on 11 degrees of freedom below
    11 + 5 sqrt(22) ~ 34.5, the margin of the S15 law test.  (The seed is not searched.)"""
    x = [0.5, 3.0, math.nan, -1.0, 8.0, 2.0]
    st = [0, 1, 1, 0, 1, 0]
    pl = ve.plan(x, st, 2)
    assert pl["n"] == [3, 2]
    P, outcomes = 24000, {}
    for pi in range(P):
        row = ve.perm_row(1, 0, pi, pl)
        assert row[2] == 0
        key = tuple(r for r, v in zip(row, pl["valid"]) if v)
        outcomes[key] = outcomes.get(key, 0) + 1
    assert len(outcomes) == 12
    exp = P / 12.0
    chi2 = sum((c - exp) ** 2 / exp for c in outcomes.values())
    print("chi2 = %.2f on 11 degrees of freedom" % chi2)
    assert chi2 < 11 + 5 * (2 * 11) ** 0.5


def test_r_composes_over_batches():
    rng = np.random.default_rng(8)
    N, G, P, S = 30, 9, 40, 3
    x, st = _trait(rng, N, S)
    pl = ve.plan(x, st, S)
    genes = _genes(rng, G, N)
    d_obs = [ve.statistic(g, pl)[0] for g in genes]
    rows = [ve.perm_row(11, 0, pi, pl) for pi in range(P)]
    whole = ve.r_counts(genes, rows, d_obs)
    parts = [ve.r_counts(genes, rows[:25], d_obs), ve.r_counts(genes, rows[25:], d_obs)]
    assert whole == [a + b for a, b in zip(*parts)] and 0 < sum(whole) < G * P


def test_host_ranking_is_the_restatements():
    from scoary_amd.engine import vanelteren_rows
    rng = np.random.default_rng(3)
    N, S = 90, 6
    st = rng.integers(0, S - 1, N)                          # the last stratum is empty
    st[:2] = S - 1
    vals = np.stack([rng.integers(0, 6, N).astype(float), rng.standard_normal(N), np.full(N, 1.5),
                     np.round(rng.standard_normal(N), 1)])
    vals[1, ::7] = np.nan
    vals[3, st == 2] = np.nan                               # a stratum without a value
    vals[0, 1] = np.nan                                     # ... and one with exactly one
    score, l, valid, w, n, tiesum, groups, c = vanelteren_rows(vals, st, S)
    for t in range(4):
        pl = ve.plan([float(v) for v in vals[t]], [int(s) for s in st], S)
        assert list(score[t]) == pl["score"] and list(valid[t]) == [bool(v) for v in pl["valid"]]
        k = len(pl["L"])
        assert list(l[t, :k]) == pl["L"] and not l[t, k:].any()
        assert list(w[t]) == pl["w"] and list(n[t]) == pl["n"] and list(tiesum[t]) == pl["tiesum"]
        assert [float(v) for v in c[t]] == pl["c"]
