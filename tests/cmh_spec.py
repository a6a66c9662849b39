"""Spec S10 in plain Python floats: the Cochran-Mantel-Haenszel statistic over per-stratum
2x2 tables, the Mantel-Haenszel odds ratio and the rejection region of the pooled count -- the same operations in
the same order as the specification, written from it and independently of the kernel.  Also the EXACT rule of
the region with fractions.Fraction.  A helper, not a test."""
import math
from fractions import Fraction

TAU = 1e-6

# UC Berkeley admissions 1973 (R's UCBAdmissions), admitted x sex in the six departments, as (a, b, c, d)
UCB = {"A": (512, 313, 89, 19), "B": (353, 207, 17, 8), "C": (120, 205, 202, 391),
       "D": (138, 279, 131, 244), "E": (53, 138, 94, 299), "F": (22, 351, 24, 317)}


def tables_abcd(rows):
    return [(a, a + c, a + b, a + b + c + d) for a, b, c, d in rows]


def cmh(tables):
    """``tables``: one (a, m, k, n) per stratum in ascending stratum order -- a = gene & label, m = gene & valid,
    k = positives, n = valid isolates of the stratum.  Returns a dict: stat, p, odds, e2, var (floats), a (the
    pooled count) and crit = (base, span)."""
    A, K, E2, V, R, Q = 0, 0, 0.0, 0.0, 0.0, 0.0
    for a, m, k, n in tables:
        if n == 0:
            continue
        b, c, d = k - a, m - a, n - k - m + a
        A += a
        K += k
        E2 += float(2 * k * m) / float(n)
        if n >= 2:
            V += ((float(k) * float(n - k)) * (float(m) * float(n - m))) / ((float(n) * float(n)) * float(n - 1))
        R += float(a * d) / float(n)
        Q += float(b * c) / float(n)
    if Q != 0.0:
        odds = R / Q
    else:
        odds = math.inf if R > 0.0 else math.nan
    out = {"a": A, "e2": E2, "var": V, "odds": odds}
    if V == 0.0:
        out.update(stat=math.nan, p=1.0, crit=(0, 0))
        return out
    delta = abs(float(A) - 0.5 * E2)
    y = min(0.5, delta)
    stat = ((delta - y) * (delta - y)) / V
    out.update(stat=stat, p=math.erfc(math.sqrt(stat / 2.0)), crit=region(A, E2, K))
    return out


def region(A, E2, K):
    """(base, span) of S10 from the pooled count, twice its expectation and the positives K of the counted strata
    (V != 0)."""
    diff = 2.0 * float(A) - E2
    if diff > TAU:
        lo, hi = math.floor((E2 - float(A)) + TAU) + 1, A - 1
    elif diff < -TAU:
        lo, hi = A + 1, math.ceil((E2 - float(A)) - TAU) - 1
    else:
        return (0, 0)
    lo, hi = max(lo, 0), min(hi, K)
    return (lo, hi - lo + 1) if hi >= lo else (0, 0)


def in_region(crit, a):
    """The test the permutation kernels make: (uint32)(a - base) >= span."""
    return ((a - crit[0]) & 0xffffffff) >= crit[1]


def exact(tables):
    """(A, E, V) as Fractions."""
    A, E, V = 0, Fraction(0), Fraction(0)
    for a, m, k, n in tables:
        if n == 0:
            continue
        A += a
        E += Fraction(k * m, n)
        if n >= 2:
            V += Fraction(k * (n - k) * m * (n - m), n * n * (n - 1))
    return A, E, V


def exact_extreme(tables, a_perm):
    """The exact rule: a permuted pooled count is as or more extreme iff |a' - E| >= |A - E| (everything is, when no
    stratum is informative)."""
    A, E, V = exact(tables)
    return V == 0 or abs(a_perm - E) >= abs(A - E)


def support(tables):
    """[lo, hi] of the pooled count under within-stratum shuffles: the sum of the strata's hypergeometric supports."""
    lo = hi = 0
    for _a, m, k, n in tables:
        if n == 0:
            continue
        lo += max(0, k + m - n)
        hi += min(k, m)
    return lo, hi
