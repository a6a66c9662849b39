"""Spec S10 on the CPU: the plain-Python restatement (tests/cmh_spec.py) against a published anchor, and its
rejection region against the exact rule in rational arithmetic."""
import math
import random
from fractions import Fraction

import numpy as np

import cmh_spec as S

def test_ucb_admissions_anchor():
    """R: mantelhaen.test(UCBAdmissions) -> X-squared = 1.4269, p-value = 0.2323, common odds ratio 0.9047."""
    r = S.cmh(S.tables_abcd(S.UCB.values()))
    for got, want in ((r["stat"], 1.4269462285866712), (r["p"], 0.23226346281705096),
                      (r["odds"], 0.9046968282586231)):
        assert abs(got - want) <= 1e-12 * want
    assert round(r["stat"], 4) == 1.4269 and round(r["p"], 4) == 0.2323 and round(r["odds"], 4) == 0.9047
    assert r["a"] == sum(t[0] for t in S.UCB.values())


def test_region_equals_the_exact_rule_on_every_small_margin_set():
    """Every margin set of 1-3 strata with n_s <= 6.  Region and exact rule are functions of (A, E, a') alone, so
    the sets are reduced to their distinct (E2 as the spec sums it, 60 E as an integer) and every pooled count A and
    permuted count a' any of the sets can reach is tried for each."""
    kinds = [(0, 0, 0)] + [(n, k, m) for n in range(1, 7) for k in range(n + 1) for m in range(n + 1)]
    n, k, m = (np.array(x, dtype=np.int64) for x in zip(*kinds))
    with np.errstate(invalid="ignore", divide="ignore"):
        e2 = np.where(n > 0, (2 * k * m).astype(np.float64) / n.astype(np.float64), 0.0)    # one rounding, as S10
    e60 = np.where(n > 0, 60 * k * m // np.maximum(n, 1), 0)                               # 60 = lcm(1 .. 6): exact
    assert all(60 * kk * mm % nn == 0 for nn, kk, mm in kinds if nn)
    inf = (n >= 2) & (k > 0) & (k < n) & (m > 0) & (m < n)                                 # the stratum adds to V
    i, j, l = np.meshgrid(*(np.arange(len(kinds)),) * 3, indexing="ij")
    keep = ((i <= j) & (j <= l) & (inf[i] | inf[j] | inf[l])).ravel()                      # ascending strata, V != 0
    i, j, l = i.ravel()[keep], j.ravel()[keep], l.ravel()[keep]
    pairs = {(float(x), int(y)) for x, y in zip((e2[i] + e2[j]) + e2[l], e60[i] + e60[j] + e60[l])}
    assert len(pairs) > 300
    top = 3 * 6
    bad = 0
    for E2, E60 in pairs:
        for A in range(top + 1):
            crit = S.region(A, E2, top)
            for ap in range(top + 1):
                bad += S.in_region(crit, ap) != (abs(60 * ap - E60) >= abs(60 * A - E60))
    assert bad == 0


def random_problem(rng, max_strata, max_n):
    tabs = []
    for _ in range(rng.randint(1, max_strata)):
        n = rng.randint(1, max_n)
        k, m = rng.randint(0, n), rng.randint(0, n)
        tabs.append((rng.randint(max(0, k + m - n), min(k, m)), m, k, n))
    return tabs


def test_region_equals_the_exact_rule_on_random_small_problems():
    rng = random.Random(10)
    pairs = 0
    for _ in range(20000):
        tabs = random_problem(rng, 4, 9)
        crit = S.cmh(tabs)["crit"]
        lo, hi = S.support(tabs)
        for ap in range(lo, hi + 1):
            assert S.in_region(crit, ap) == S.exact_extreme(tabs, ap), (tabs, ap)
            pairs += 1
    assert pairs > 40000


def test_region_is_a_superset_of_the_exact_rule_on_large_strata():
    """Up to 40 strata of up to 2000 isolates: the integers next to the mirror image 2E - A of the observed count
    (where the two rules can part) and the ends of the support.  Every exactly extreme count is in the region; a
    count in the region that is not exactly extreme has its distance within tau (plus the fp64 error of E2, below
    2e-8 by S10's bound) of the observed one."""
    rng = random.Random(11)
    slack = Fraction(S.TAU) + Fraction(2, 10 ** 8)
    differ = 0
    for _ in range(600):
        tabs = random_problem(rng, 40, 2000)
        A, E, V = S.exact(tabs)
        crit = S.cmh(tabs)["crit"]
        lo, hi = S.support(tabs)
        mirror = math.floor(2 * E - A)
        for ap in {lo, hi, A} | set(range(mirror - 2, mirror + 4)):
            if not lo <= ap <= hi:
                continue
            ex, got = S.exact_extreme(tabs, ap), S.in_region(crit, ap)
            assert got or not ex, (tabs, ap)
            if got != ex:
                differ += 1
                assert abs(abs(ap - E) - abs(A - E)) <= slack, (tabs, ap)
    # exact ties on purpose: two equal strata mirrored around E
    for n, k, m in ((7, 3, 4), (1999, 1000, 37), (12, 6, 6)):
        lo, hi = max(0, k + m - n), min(k, m)
        for a1 in range(lo, hi + 1):
            for a2 in range(lo, hi + 1):
                tabs = [(a1, m, k, n), (a2, m, k, n)]
                crit = S.cmh(tabs)["crit"]
                A, E, V = S.exact(tabs)
                tie = 2 * E - A
                if tie.denominator == 1 and 2 * lo <= tie <= 2 * hi and V != 0:
                    assert S.in_region(crit, int(tie)) and S.in_region(crit, A)


def test_degenerate_cases():
    # no informative stratum: the gene in every (or no) isolate of every stratum, or a constant trait
    for tabs in ([(3, 5, 3, 5), (0, 4, 0, 4)], [(0, 0, 2, 6)], [(1, 1, 1, 1), (0, 0, 1, 1)], []):
        r = S.cmh(tabs)
        assert r["var"] == 0.0 and math.isnan(r["stat"]) and r["p"] == 1.0 and r["crit"] == (0, 0)
        assert all(S.in_region(r["crit"], a) for a in range(0, 12))
    # a stratum of one isolate adds to A, E2, R and Q but never to V (n - 1 = 0 is not divided by)
    base = [(2, 4, 3, 8)]
    r0, r1 = S.cmh(base), S.cmh(base + [(1, 1, 1, 1)])
    assert r1["var"] == r0["var"] and r1["a"] == r0["a"] + 1 and r1["e2"] == r0["e2"] + 2.0
    assert r1["stat"] == r0["stat"] and r1["odds"] == r0["odds"]
    # a stratum emptied by the mask is skipped
    assert S.cmh(base + [(0, 0, 0, 0)]) == S.cmh(base) == S.cmh([(0, 0, 0, 0)] + base)
    # A exactly at E: nothing is less extreme, stat = 0, p = 1
    r = S.cmh([(2, 4, 4, 8)])
    assert r["e2"] == 4.0 and r["stat"] == 0.0 and r["p"] == 1.0 and r["crit"] == (0, 0)
    # half a count from E: inside the continuity correction stat = 0 as well; a' = 1 is exactly as far, a tie
    r = S.cmh([(2, 3, 4, 8)])
    assert r["stat"] == 0.0 and r["p"] == 1.0 and r["crit"] == (0, 0)
    # one and a half counts from E = 1.5: only 1 and 2 are less extreme
    assert S.cmh([(3, 3, 4, 8)])["crit"] == (1, 2) == S.cmh([(0, 3, 4, 8)])["crit"]
    # odds: inf when only Q vanishes, nan when both do
    assert S.cmh([(3, 3, 3, 8)])["odds"] == math.inf and math.isnan(S.cmh([(0, 0, 3, 8)])["odds"])
