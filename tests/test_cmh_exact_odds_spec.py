"""Spec S13 on the host: the floating-point restatement of the conditional odds ratio and its exact confidence limits
(cmh_exact_odds_spec.py) against the exact bracketing check in integers, on every small margin set at every count of
its support and on random problems at three levels; the special values, the order of the three numbers, their
agreement with the one-sided exact tests, and one stratum against SciPy."""
import math
from fractions import Fraction
from itertools import product

import numpy as np
import pytest

import cmh_exact_odds_spec as S13
import cmh_exact_spec as S12
import cmh_spec as S10
from test_cmh_exact_spec import _with_a

LEVELS = (0.5, 0.95, 0.999)
EPS = 1e-12


def _side_of_one(odds, xa, E):
    """odds > 1 exactly when A > E and odds < 1 exactly when A < E; at A = E the exact root is 1 and a double within
    1e-12 of it may fall on either side."""
    return abs(odds - 1.0) <= EPS if xa == E else (odds > 1) == (xa > E) and (odds < 1) == (xa < E)


def _check_counts(shapes, half, worst):
    """Every count of the support as the observed one: the restatement against ``brackets`` at 1e-12, the special
    values, the order and the one-sided tests.  Returns the number of roots checked."""
    zero = [(0,) + s for s in shapes]
    lo, W, D = S12.exact_weights(zero)
    flo, f = S12.float_pmf(zero)
    assert flo == lo and len(f) == len(W)
    L, got = len(W), S13.restate_counts(f, half)
    if L == 1:
        assert math.isnan(got[0, 0]) and got[1, 0] == 0.0 and got[2, 0] == math.inf
        return 0
    E = Fraction(sum(i * w for i, w in enumerate(W)), D)
    roots = 0
    for i in range(L):
        tables = _with_a(shapes, lo + i)
        odds, lower, upper = got[:, i]
        assert not np.isnan(got[:, i]).any() and lower <= odds <= upper, (shapes, i, got[:, i])
        for which, v in zip(S13.WHICH, (odds, lower, upper)):
            want = S13.special(tables, which)
            if want is not None:
                assert v == want, (shapes, i, which, v)
                continue
            err = S13.error_within(tables, half, float(v), which, EPS, (lo, W, D))
            assert err <= EPS, (shapes, i, which, v)
            worst[0] = max(worst[0], err)
            roots += 1
        assert _side_of_one(odds, i, E), (shapes, i, odds)
        ge, le = Fraction(sum(W[i:]), D), Fraction(sum(W[:i + 1]), D)
        h = Fraction(half)
        if abs(ge - h) > h / 10 ** 9:
            assert (lower > 1) == (ge < h), (shapes, i, lower)
        if abs(le - h) > h / 10 ** 9:
            assert (upper < 1) == (le < h), (shapes, i, upper)
    return roots


def test_every_small_margin_set_at_every_count_against_the_exact_check():
    """1 and 2 strata with n_s <= 5 (S12's 8372 problems), level 0.95."""
    one = [(m, k, n) for n in range(0, 6) for k in range(n + 1) for m in range(n + 1)]
    worst, roots, problems = [0.0], 0, 0
    for shapes in [(s,) for s in one] + list(product(one, one)):
        roots += _check_counts(list(shapes), S13.half_of(0.95), worst)
        problems += 1
    print("%d problems, %d roots, every one within %.0e of the exact root" % (problems, roots, worst[0]))
    assert problems == 8372 and roots > 10000 and worst[0] <= EPS


@pytest.mark.parametrize("level", LEVELS)
def test_random_problems_against_the_exact_check(level):
    """2000 random problems of 1 to 8 strata with n_s < 70, split over the three levels; every value by ``brackets``
    at 1e-12, the order of the three numbers and their agreement with E and with the one-sided exact tests."""
    rng = np.random.default_rng(int(level * 1000))
    half, h = S13.half_of(level), Fraction(S13.half_of(level))
    worst, roots, count = 0.0, 0, {0.5: 667, 0.95: 667, 0.999: 666}[level]
    for _ in range(count):
        tables = S12.random_tables(rng, int(rng.integers(1, 9)), 70)
        weights = lo, W, D = S12.exact_weights(tables)
        xa = S10.cmh(tables)["a"] - lo
        got = S13.restate(tables, half)
        for which, v in zip(S13.WHICH, got):
            want = S13.special(tables, which)
            if want is not None:
                assert v == want or (math.isnan(v) and math.isnan(want)), (tables, which, v)
                continue
            err = S13.error_within(tables, half, v, which, EPS, weights)
            assert err <= EPS, (tables, which, v)
            worst = max(worst, err)
            roots += 1
        if len(W) == 1:
            continue
        odds, lower, upper = got
        E = Fraction(sum(i * w for i, w in enumerate(W)), D)
        assert lower <= odds <= upper and _side_of_one(odds, xa, E), (tables, got)
        ge, le = S13.one_sided(tables)
        if abs(ge - h) > h / 10 ** 9:
            assert (lower > 1) == (ge < h), (tables, lower)
        if abs(le - h) > h / 10 ** 9:
            assert (upper < 1) == (le < h), (tables, upper)
    print("level %s: %d problems, %d roots, every one within %.0e of the exact root" % (level, count, roots, worst))
    assert roots > count and worst <= EPS


def test_special_values_are_exact():
    half = S13.half_of(0.95)
    nan_lo_hi = S13.restate([(0, 0, 2, 5), (1, 1, 1, 1), (0, 3, 0, 4)], half)          # no informative stratum
    assert math.isnan(nan_lo_hi[0]) and nan_lo_hi[1:] == (0.0, math.inf)
    at_lo = S13.restate([(0, 3, 2, 6), (1, 4, 3, 6)], half)                            # A = lo = 0 + 1
    assert at_lo[0] == 0.0 and at_lo[1] == 0.0 and 0.0 < at_lo[2] < math.inf
    at_hi = S13.restate([(2, 3, 2, 6), (3, 4, 3, 6)], half)                            # A = hi = 2 + 3
    assert at_hi[0] == math.inf and at_hi[2] == math.inf and 0.0 < at_hi[1] < math.inf
    for tables, got in (([(0, 3, 2, 6), (1, 4, 3, 6)], at_lo), ([(2, 3, 2, 6), (3, 4, 3, 6)], at_hi)):
        for which, v in zip(S13.WHICH, got):
            assert S13.special(tables, which) in (None, v)
    # the mirrored problem has the reciprocal numbers
    mirror = S13.restate([(3, 3, 4, 6), (3, 4, 3, 6)], half)
    assert mirror[0] == math.inf and at_lo[2] * mirror[1] == pytest.approx(1.0, rel=1e-12)


def test_one_stratum_against_scipy():
    """200 random 2 x 2 tables with n < 200 against scipy.stats.contingency.odds_ratio(kind="conditional") and its
    confidence_interval(0.95): SciPy's root finder (brentq with an absolute xtol of 2e-12) is the looser side, and the
    looser the smaller the root -- at the level 0.999 a lower limit of 2e-6 differs by 1.2e-9 relative.  Measured over
    this sample: worst relative difference 4.25e-12, at a lower limit of 0.0051 (restate itself is within 1e-14 of the
    exact roots, above); the bound is ten times that."""
    from scipy.stats.contingency import odds_ratio
    rng = np.random.default_rng(200)
    worst, done = 0.0, 0
    while done < 200:
        n = int(rng.integers(2, 200))
        k, m = int(rng.integers(1, n)), int(rng.integers(1, n))
        a = int(rng.integers(max(0, k + m - n), min(k, m) + 1))
        level = 0.95
        got = S13.restate([(a, m, k, n)], S13.half_of(level))
        res = odds_ratio([[a, k - a], [m - a, n - k - m + a]], kind="conditional")
        ci = res.confidence_interval(level)
        want = (res.statistic, ci.low, ci.high)
        done += 1
        if math.isnan(got[0]):
            assert math.isnan(want[0])
            continue
        for g, w in zip(got, want):
            if g == 0.0 or math.isinf(g):
                assert g == w, (a, m, k, n, got, want)
            else:
                worst = max(worst, abs(g - w) / g)
    print("one stratum against SciPy: worst relative difference %.2e over %d tables" % (worst, done))
    assert worst <= 4.25e-11
