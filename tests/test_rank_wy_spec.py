"""Spec S17's restatement (rank_wy_spec.py) against the properties the spec states: s is strictly increasing in E,
stands for the p of S15 / S16, and the counts r_fwer dominate the per-gene counts, meet them at G = 1, are P where a
gene cannot be tested or its |D| is within the continuity constant, and compose over permutation batches."""
import math

import numpy as np
import pytest

import rank_wy_spec as wy
import ranksum_spec as rsp
import vanelteren_spec as vsp

SEED = 0x5EED5EED1234


def _values(rng, N, ties, missing):
    x = np.round(rng.standard_normal(N), 1 if ties else 6)
    if missing:
        x[rng.random(N) < 0.2] = np.nan
    return x


def _genes(rng, G, N):
    genes = (rng.random((G, N)) < rng.uniform(0.1, 0.9, (G, 1))).astype(np.int64)
    if G > 2:
        genes[1] = 0                                    # untestable: m = 0
        genes[2] = 1                                    # untestable: m = n
    return genes


def _real_ivs():
    """iv of every testable gene of a few real plans of both tests, and the extremes of the kernels' range."""
    rng = np.random.default_rng(17)
    ivs = set()
    for N in (5, 9, 40):
        genes = _genes(rng, 12, N)
        vals = _values(rng, N, True, True)
        ivs.update(wy.ranksum_problem(genes, vals)["iv"])
        ivs.update(wy.vanelteren_problem(genes, vals, rng.integers(0, 3, N), 3)["iv"])
    ivs.discard(0.0)
    n = rsp.MAX_ISOLATES                                # the largest and the smallest variance of S15
    ivs.add(wy.inverse(wy.var_ranksum(n // 2, n, 0)))
    ivs.add(wy.inverse(wy.var_ranksum(1, 2, 0)))
    return sorted(ivs)


def test_s_is_nonnegative_and_strictly_increasing_in_e():
    ivs = _real_ivs()
    assert len(ivs) > 20 and min(ivs) > 0
    # every E of a small n: |D| <= n (n - 1) for S15, and 16 319 n under S16's weights; and the top of the range
    small = np.arange(0, 16319 * 9 + 2, dtype=np.int64)
    top = np.arange(wy.MAX_E - 4000, wy.MAX_E + 1, dtype=np.int64)
    assert wy.MAX_E == 266326080 < 2 ** 28
    for cc in (0, 1):
        for iv in ivs:
            for E in (small, top):
                D = E + cc                                              # |D| = E + cc, as far as |D| goes
                s = wy.stats(D[None, D <= wy.MAX_E], cc, [iv])[0]
                assert s[0] >= 0 and (np.diff(s) > 0).all(), (cc, iv)
            assert wy.stat(cc, cc, iv) == 0.0 == wy.stat(0, cc, iv) and wy.stat(-7, cc, iv) == wy.stat(7, cc, iv)
    # an untestable gene: the identity of the maximum in every row
    assert not wy.stats(top[None, :], 0, [0.0]).any()
    # the scalar and the array form are one function
    for D in (0, 1, -1, 2, 12345, -wy.MAX_E):
        assert wy.stat(D, 1, ivs[3]) == wy.stats([[D]], 1, [ivs[3]])[0, 0]


def test_s_stands_for_the_p_of_both_tests():
    """erfc(sqrt(s / 4) / sqrt 2) against the restatements' p: 1e-12 relative where p > 1e-280, the margin those
    restatements are themselves held to against SciPy."""
    rng = np.random.default_rng(3)
    worst, seen, deep = 0.0, 0, 0
    cases = [(N, True) for N in (6, 13, 60, 300)] + [(1500, False)]
    for N, ties in cases:
        genes = _genes(rng, 30, N)
        vals = _values(rng, N, ties, True)
        genes[0] = np.nan_to_num(vals, nan=-9.0) > np.nanmedian(vals)   # a driver gene: a deep tail
        pr = wy.ranksum_problem(genes, vals)
        S = 4
        strata = rng.integers(0, S, N)
        pv = wy.vanelteren_problem(genes, vals, strata, S)
        for g in range(len(genes)):
            ok, _auc, p = rsp.tail(pr["d"][g], pr["m"][g], pr["n"], pr["tiesum"])
            assert ok == (pr["iv"][g] > 0)
            ok2, var2, _den, _auc2, p2 = vsp.tail(pv["d"][g], pv["ms"][g], pv["pl"])
            assert ok2 == (pv["iv"][g] > 0) and (not ok2 or var2 == pv["var"][g])
            for okk, want, s in ((ok, p, pr["s_obs"][g]), (ok2, p2, pv["s_obs"][g])):
                if not okk:
                    assert s == 0.0 and want == 1.0
                elif want > 1e-280:
                    seen += 1
                    deep += want < 1e-100
                    worst = max(worst, abs(wy.p_of(s) - want) / want)
    print("%d testable cells, %d below 1e-100, worst relative difference %.3g" % (seen, deep, worst))
    assert seen > 200 and deep >= 1 and worst <= 1e-12


def _problem(rng, k):
    """The k-th random small problem: (kind, genes, D_obs, cc, iv, s_obs, D [G, P]) with the rows of the spec's own
    permutation law."""
    N = int(rng.integers(3, 15))
    G = 1 if k % 10 == 0 else int(rng.integers(2, 9))
    P = int(rng.integers(5, 14))
    genes = _genes(rng, G, N)
    vals = _values(rng, N, ties=k % 2 == 0, missing=k % 3 == 0)
    if k % 4 < 2:
        pr = wy.ranksum_problem(genes, vals)
        rows = [rsp.perm_row(SEED + k, 0, pi, pr["valid"], pr["rc"]) for pi in range(P)]
        return "ranksum", genes, pr, wy.permuted(genes, rows)
    S = int(rng.integers(1, 5))
    strata = rng.integers(0, S, N)
    strata[:min(3, N)] = [0, S - 1, S - 1][:min(3, N)]               # strata of size 1 and 2 occur by themselves too
    pv = wy.vanelteren_problem(genes, vals, strata, S)
    rows = [vsp.perm_row(SEED + k, 0, pi, pv["pl"]) for pi in range(P)]
    return "vanelteren", genes, pv, wy.permuted(genes, rows)


def test_r_fwer_dominates_r_and_meets_it_for_one_gene():
    rng = np.random.default_rng(2024)
    kinds, singles, sizes, strict, capped = set(), 0, set(), 0, 0
    for k in range(200):
        kind, genes, pr, D = _problem(rng, k)
        G, P = D.shape
        kinds.add(kind)
        if kind == "vanelteren":
            sizes.update(pr["pl"]["n"])
        mx = wy.maxs(D, pr["cc"], pr["iv"])
        rf, r = wy.r_fwer(mx, pr["s_obs"]), wy.r_count(D, pr["d"])
        assert (rf >= r).all(), (k, rf, r)
        strict += int((rf > r).sum())
        if G == 1:
            singles += 1
            assert (rf == r).all(), (k, rf, r)
        for g in range(G):                               # untestable, or |D_obs| within the continuity constant
            if pr["iv"][g] == 0.0 or abs(pr["d"][g]) <= pr["cc"]:
                capped += 1
                assert rf[g] == P and pr["s_obs"][g] == 0.0, (k, g)
        # the counts per gene, restated once more through s: the law r_fwer is built on
        for g in range(G):
            if pr["iv"][g] > 0:
                assert r[g] == (wy.stats(D[g:g + 1], pr["cc"], [pr["iv"][g]])[0] >= pr["s_obs"][g]).sum()
    assert kinds == {"ranksum", "vanelteren"} and singles == 20 and {1, 2} <= sizes and strict > 50 and capped > 100


def test_maxs_composes_over_batches():
    rng = np.random.default_rng(99)
    for k in (1, 2, 3, 6, 7):
        _kind, _genes_, pr, D = _problem(rng, k)
        P = D.shape[1]
        cut = P // 2
        whole = wy.maxs(D, pr["cc"], pr["iv"])
        parts = np.concatenate([wy.maxs(D[:, :cut], pr["cc"], pr["iv"]), wy.maxs(D[:, cut:], pr["cc"], pr["iv"])])
        assert np.array_equal(whole, parts)
        # and by max over gene shards, which the stage does not use
        if D.shape[0] > 1:
            h = D.shape[0] // 2
            assert np.array_equal(whole, np.maximum(wy.maxs(D[:h], pr["cc"], pr["iv"][:h]),
                                                    wy.maxs(D[h:], pr["cc"], pr["iv"][h:])))
        assert np.array_equal(wy.r_fwer(whole, pr["s_obs"]),
                              wy.r_fwer(parts[:cut], pr["s_obs"]) + wy.r_fwer(parts[cut:], pr["s_obs"]))


def test_the_variance_is_the_observed_tests_own():
    """var_ranksum restates the expression inside ranksum_spec.tail: the p rebuilt from it is tail's, bit for bit."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(2, 60))
        m = int(rng.integers(0, n + 1))
        tiesum = int(rng.choice([0, 6, 24, n ** 3 - n]))
        D = int(rng.integers(-m * (n - m) - 1, m * (n - m) + 2))
        ok, _auc, p = rsp.tail(D, m, n, tiesum)
        var = wy.var_ranksum(m, n, tiesum)
        assert ok == (var > 0)
        if ok:
            z = max(0.0, abs(D) * 0.5 - 0.5) / math.sqrt(var)
            assert math.erfc(z / math.sqrt(2.0)) == p
    assert wy.inverse(0.0) == 0.0 and wy.inverse(4.0) == 0.25


@pytest.mark.parametrize("cc", (0, 1))
def test_equal_e_ties_exactly(cc):
    iv = wy.inverse(wy.var_ranksum(7, 20, 6))
    for E in (1, 2, 77, 266326079):
        assert wy.stat(E + cc, cc, iv) == wy.stat(-(E + cc), cc, iv) == wy.stats([[E + cc]], cc, [iv])[0, 0]
