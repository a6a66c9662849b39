"""Spec S12 on the host: the floating-point restatement of the exact conditional test (cmh_exact_spec.py) against the
exact one in integers and Fractions, on every small margin set and on random problems; one stratum against the
oracle's Fisher p; and the laws that do hold between p, p_region and the pmf (p_region <= p is not one of them)."""
from fractions import Fraction
from itertools import product

import numpy as np

import cmh_exact_spec as S12
import cmh_spec as S10


def _with_a(shapes, A):
    """Per-stratum (a, m, k, n) with the pooled count A: the surplus over the lower ends handed out in order."""
    rest, out = A - sum(max(0, k + m - n) for m, k, n in shapes if n > 0), []
    for m, k, n in shapes:
        lo_s, hi_s = (max(0, k + m - n), min(k, m)) if n > 0 else (0, 0)
        take = min(rest, hi_s - lo_s) if n > 0 else 0
        rest -= take
        out.append((lo_s + take, m, k, n))
    assert rest == 0
    return out


def _check_problem(shapes, worst):
    """Every count of the support as the observed one: table, p, p_region and the laws.  Returns whether the problem
    has a near-tie (its table is then held at the counts that no near-tie touches -- here: skipped)."""
    lo, W, D = S12.exact_weights([(0,) + s for s in shapes])
    if S12.near_tie(W):
        return True
    want_tab = np.array([float(p) for p in S12.exact_p_table(W, D)])
    flo, f = S12.float_pmf([(0,) + s for s in shapes])
    assert flo == lo and len(f) == len(W)
    assert abs(float(f.sum()) - 1.0) <= 1e-13
    got_tab = S12.float_p_table(f)
    err = np.abs(got_tab - want_tab)
    worst[0] = max(worst[0], float((err / want_tab).max()))
    assert err.max() <= 1e-12 and (err <= 1e-12 * want_tab).all()
    for i in range(len(W)):
        tables = _with_a(shapes, lo + i)
        crit = S10.cmh(tables)["crit"]
        want_region = float(S12.exact_region(lo, W, D, crit))
        got_region = S12.float_region(lo, f, crit)
        assert abs(got_region - want_region) <= 1e-12 * want_region
        fa = Fraction(W[i], D)
        assert S12.exact_p_table(W, D)[i] >= fa                       # p(A) >= f(A)
        assert S12.exact_region(lo, W, D, crit) >= fa                 # the region holds the observed count
        if len(W) == 1:
            assert got_tab[0] == 1.0 and got_region == 1.0
    return False


def test_every_small_margin_set_against_fractions():
    one = [(m, k, n) for n in range(0, 6) for k in range(n + 1) for m in range(n + 1)]
    worst, ties, problems = [0.0], 0, 0
    for shapes in [(s,) for s in one] + list(product(one, one)):
        ties += _check_problem(list(shapes), worst)
        problems += 1
    print("%d problems, %d with a near-tie, worst relative error %.2e" % (problems, ties, worst[0]))
    assert ties == 0


def test_random_problems_against_fractions():
    rng = np.random.default_rng(12)
    worst, ties = [0.0], 0
    for i in range(2000):
        tables = S12.random_tables(rng, int(rng.integers(1, 9)), 70)
        lo, tab, p, region, tie = S12.reference(tables)
        if tie:
            ties += 1
            continue
        glo, gtab, gp, gregion = S12.restate(tables)
        assert glo == lo
        err = np.abs(gtab - tab)
        big = tab >= S12.TINY
        worst[0] = max(worst[0], float((err[big] / tab[big]).max()))
        assert err.max() <= 1e-12 and (err[big] <= 1e-12 * tab[big]).all() and (gtab[~big] <= S12.TINY).all()
        assert abs(gregion - region) <= 1e-12 * max(region, S12.TINY) and abs(gp - p) <= 1e-12 * max(p, S12.TINY)
    print("2000 problems, %d with a near-tie, worst relative error %.2e" % (ties, worst[0]))
    assert ties <= 20                                                   # at most 1 %


def test_one_stratum_is_fishers_exact_test():
    from oracle import oracle as orc
    rng = np.random.default_rng(1)
    tabs, got = [], []
    for _ in range(300):
        (a, m, k, n), = S12.random_tables(rng, 1, 400)
        if n == 0:
            continue
        tabs.append((a, k - a, m - a, n - k - m + a))              # (tp gp, tp gn, tn gp, tn gn) = a, b, c, d
        got.append(S12.restate([(a, m, k, n)])[2])
    _odds, p = orc.fisher_many(np.array(tabs, dtype=np.int64))
    err = np.abs(np.array(got) - p)
    print("one stratum against the oracle's Fisher p: max abs error %.2e" % err.max())
    assert err.max() <= 1e-12


def test_region_mass_is_not_bounded_by_p():
    """The CMH region orders the counts by distance from the mean, the exact p by probability: on a skewed pmf
    either may be the larger.  What the tests may rely on is asserted in _check_problem; here: both orders occur."""
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(400):
        tables = S12.random_tables(rng, int(rng.integers(1, 5)), 30)
        _lo, _tab, p, region, _tie = S12.reference(tables)
        seen.add(np.sign(region - p))
    assert {-1.0, 1.0} <= seen
