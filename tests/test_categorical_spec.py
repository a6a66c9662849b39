"""Spec S20's plain-Python restatement (categorical_spec.py) against exact rationals and SciPy, its two routes to the
exceedance decision on real ties, the K = 2 reduction, every untestable branch and the law of the shuffle.  CPU only."""
import itertools
import math
import random
from fractions import Fraction

import numpy as np
import pytest
from scipy import stats

import categorical_spec as cs

TIES_333 = dict(nk=[3, 3, 3], m=4, vectors=[(1, 1, 2), (2, 1, 1)])
TIES_6312 = dict(nk=[6, 3, 12], m=8, vectors=[(1, 2, 5), (3, 0, 5), (3, 2, 3)])


def _random_table(rng, K, nmax):
    nk = [rng.choice([0, rng.randint(1, nmax)]) if rng.random() < 0.15 else rng.randint(1, nmax) for _ in range(K)]
    a = [rng.randint(0, x) for x in nk]
    return nk, a


def test_x2_is_within_its_rounding_bound_of_the_exact_value():
    """2K + 3 roundings (one per conversion of c_k^2, one per division, K - 1 additions, the product m (n - m) and
    the last division), each <= 2^-53 relative on positive terms, doubled for the second-order terms."""
    rng = random.Random(20)
    checked = 0
    for _ in range(3000):
        K = rng.randint(2, 8)
        nk, a = _random_table(rng, K, rng.choice([5, 60, 2000, 16320 // K]))
        ok, x2, df, p, v = cs.statistic(a, nk)
        if not ok:
            continue
        exact = cs.x2_exact(a, nk)
        if exact == 0:
            assert x2 == 0.0
            continue
        assert abs(Fraction(x2) - exact) / exact <= Fraction(4 * K + 16, 1 << 53), (nk, a)
        assert v == math.sqrt(x2 / float(sum(nk))) and df == sum(1 for x in nk if x > 0) - 1
        checked += 1
    assert checked > 2500


def test_x2_and_p_are_scipys_chi2_contingency():
    rng = random.Random(21)
    checked = small = 0
    for _ in range(600):
        K = rng.randint(2, 8)
        nk, a = _random_table(rng, K, rng.choice([4, 30, 400, 2000]))
        ok, x2, df, p, v = cs.statistic(a, nk)
        if not ok:
            continue
        tab = np.array([[x for x, n in zip(a, nk) if n > 0], [n - x for x, n in zip(a, nk) if n > 0]])
        want = stats.chi2_contingency(tab, correction=False)
        assert want.dof == df
        assert abs(x2 - want.statistic) <= 1e-12 * want.statistic, (nk, a)
        if want.pvalue > 1e-290:
            assert abs(p - want.pvalue) <= 1e-10 * want.pvalue, (nk, a, p, want.pvalue)
            checked += 1
            small += want.pvalue < 1e-20
    assert checked > 400 and small > 20


@pytest.mark.parametrize("family", [TIES_333, TIES_6312], ids=["3-3-3", "6-3-12"])
def test_real_ties_count_by_both_routes_and_an_fp64_sum_tells_them_apart(family):
    nk, vectors = family["nk"], family["vectors"]
    assert all(sum(v) == family["m"] and all(x <= n for x, n in zip(v, nk)) for v in vectors)
    assert len(set(cs.s_exact(v, nk) for v in vectors)) == 1
    for u, v in itertools.product(vectors, repeat=2):
        assert cs.exceeds(u, v, nk) and cs.exceeds_limbs(u, v, nk)
    # the case is a real one: the ascending-k fp64 sums of equal rationals differ, so >= in fp64 would miss a tie
    sums = [cs.s_fp64(v, nk) for v in vectors]
    assert len(set(sums)) >= 2
    lo, hi = vectors[sums.index(min(sums))], vectors[sums.index(max(sums))]
    assert not cs.s_fp64(lo, nk) >= cs.s_fp64(hi, nk) and cs.exceeds(lo, hi, nk)
    if family is TIES_333:
        assert sorted(sums) == [1.9999999999999998, 2.0]


def test_the_two_routes_agree_on_random_tables():
    rng = random.Random(22)
    ties = strict = 0
    for i in range(20000):
        K = rng.randint(1, 8)
        if i % 4 == 0:                                # a balanced design and a rearranged table: ties are common
            nk = [rng.randint(1, 16320)] * K
            a = [rng.randint(0, nk[0]) for _ in range(K)]
            b = a[:]
            rng.shuffle(b)
            if rng.random() < 0.5:
                b[rng.randrange(K)] = rng.randint(0, nk[0])
        else:
            nk, a = _random_table(rng, K, 16320)
            b = [rng.randint(0, x) for x in nk]
        want = cs.exceeds(b, a, nk)
        assert cs.exceeds_limbs(b, a, nk) == want, (nk, a, b)
        assert cs.exceeds_limbs(a, b, nk) == cs.exceeds(a, b, nk), (nk, a, b)
        ties += cs.s_exact(a, nk) == cs.s_exact(b, nk)
        strict += not want
    assert ties > 1000 and strict > 3000
    # the largest weights the limits allow: eight classes of pairwise coprime sizes just under the limit
    nk = [16319, 16318, 16317, 16315, 16313, 16311, 16309, 16307]
    assert max(cs.weights(nk)) > 1 << 90 and max(cs.weights(nk)) < 1 << 112
    for _ in range(500):
        a, b = ([rng.randint(0, x) for x in nk] for _ in range(2))
        assert cs.exceeds_limbs(b, a, nk) == cs.exceeds(b, a, nk)


def test_two_classes_are_the_two_by_two_pearson_test():
    rng = random.Random(23)
    for _ in range(2000):
        n1, n2 = rng.randint(1, 300), rng.randint(1, 300)
        n = n1 + n2
        a = [rng.randint(0, n1), rng.randint(0, n2)]
        m = sum(a)
        if not 0 < m < n:
            continue
        b, c, d = n1 - a[0], a[1], n2 - a[1]          # the 2 x 2 table (a b / c d): gene by class
        pearson = Fraction(n * (a[0] * d - b * c) ** 2, (a[0] + b) * (c + d) * (a[0] + c) * (b + d))
        assert cs.x2_exact(a, [n1, n2]) == pearson
        x = rng.randint(max(0, m - n2), min(m, n1))   # a permuted table with the same margins
        want = abs(n * x - m * n1) >= abs(n * a[0] - m * n1)
        assert cs.exceeds([x, m - x], a, [n1, n2]) == want == cs.exceeds_limbs([x, m - x], a, [n1, n2])


def test_untestable_branches_and_an_empty_class():
    untestable = (False, 0.0, None, 1.0, 0.0)
    for a, nk in (([0, 0], [0, 0]),                   # n = 0
                  ([1, 0], [1, 0]), ([0, 0], [1, 0]),  # n = 1
                  ([0, 0, 0], [3, 4, 5]),             # m = 0
                  ([3, 4, 5], [3, 4, 5]),             # m = n
                  ([2, 0, 0], [5, 0, 0]),             # K' = 1
                  ([2], [5])):                        # K = 1
        got = cs.statistic(a, nk)
        assert (got[0], got[1], got[3], got[4]) == (untestable[0], untestable[1], untestable[3], untestable[4])
        assert not cs.testable(a, nk)
    assert cs.statistic([1, 0], [1, 1])[0]            # n = 2 is the smallest testable trait
    # a class that is empty among the valid isolates: df falls by one and the class adds nothing
    full = cs.statistic([2, 3], [5, 7])
    gap = cs.statistic([2, 0, 3], [5, 0, 7])
    assert gap == full and gap[2] == 1
    classes, codes = cs.codes_of(["b", None, "a", "b", "10", "9", None])
    assert classes == ["10", "9", "a", "b"] and codes == [4, 0, 3, 4, 1, 2, 0]      # sorted as Python strings
    assert cs.sizes(codes, 4) == [1, 1, 1, 2] and cs.table([1, 1, 0, 1, 0, 1, 1], codes, 4) == [0, 1, 0, 2]
    assert cs.most_enriched([1, 2, 0, 2], [2, 4, 0, 3]) == 3 and cs.most_enriched([1, 2], [2, 4]) == 0


def test_shuffled_rows_keep_the_class_sizes_and_the_missing_isolates():
    rng = random.Random(24)
    codes = [rng.choice([0, 1, 1, 2, 3, 5]) for _ in range(90)]
    seen = set()
    for pi in range(12):
        row = cs.perm_row(0xABCDEF, 2, pi, codes)
        assert [c == 0 for c in row] == [c == 0 for c in codes]
        assert cs.sizes(row, 5) == cs.sizes(codes, 5)
        seen.add(tuple(row))
    assert len(seen) == 12 and cs.perm_row(0xABCDEF, 2, 3, codes) == cs.perm_row(0xABCDEF, 2, 3, codes)
    # the shuffle of categorical trait t is the shuffle of quantitative trait t at the same seed
    import ranksum_spec as rs
    valid = [1 if c else 0 for c in codes]
    marks = [100 + i if c else 0 for i, c in enumerate(codes)]
    moved = rs.perm_row(0xABCDEF, 2, 5, valid, marks)
    assert [codes[x - 100] if x else 0 for x in moved] == cs.perm_row(0xABCDEF, 2, 5, codes)
