"""Spec S11 on the CPU (tests/cmh_wy_spec.py, plain floats, against fractions.Fraction): the order u puts on the
pooled counts is the continuity-corrected exact rule, S10's rejection region lies inside {u(x) <= u(A)} (so
r_cmh_fwer >= r_cmh), the snap of E2 is needed for that (a named counter-example), [lo, hi] is exactly the range of
the pooled count over all within-stratum labelings, and a (trait, gene) without an informative stratum has a table
of one entry, 1.0."""
import itertools
import random
from fractions import Fraction

import numpy as np

import cmh_spec as S10
import cmh_wy_spec as S11

# (a, m, k, n) per stratum: E = 6 exactly and A = 5, so x = 7 is exactly as extreme; the fp64 sum E2 is not 12
SNAP_CASE, SNAP_X = [(3, 5, 4, 6), (1, 1, 2, 2), (0, 1, 0, 2), (1, 2, 5, 6)], 7
HALF = Fraction(1, 2)


def check_problem(tables, stats):
    """Every count of the support of one problem: u(x) <= u(A) iff the exact continuity-corrected rule, and the
    counts of S10's region among them.  Returns the number of counts."""
    r = S10.cmh(tables)
    A, E, V = S10.exact(tables)
    lo, hi = S11.support(tables)
    assert lo <= A <= hi
    u_a = S11.u_entry(A, r["e2"], r["var"])
    assert 0.0 < u_a <= 1.0
    assert S11.u_row(lo, hi, r["e2"], r["var"]).tolist() == [S11.u_entry(x, r["e2"], r["var"]) for x in range(lo, hi + 1)]
    own = max(abs(A - E) - HALF, 0)
    for x in range(lo, hi + 1):
        u_x = S11.u_entry(x, r["e2"], r["var"])
        assert 0.0 < u_x <= 1.0
        exact = V == 0 or max(abs(x - E) - HALF, 0) >= own
        assert (u_x <= u_a) == exact, (tables, x)
        if S10.in_region(r["crit"], x):
            stats["region"] += 1
            assert u_x <= u_a, (tables, x)
    return hi - lo + 1


def small_margins(nmax):
    return [(m, k, n) for n in range(nmax + 1) for k in range(n + 1) for m in range(n + 1)]


def small_problems(strata, nmax):
    """Every problem of ``strata`` strata with n_s <= nmax: all margins and all observed counts."""
    for ms in itertools.product(small_margins(nmax), repeat=strata):
        for As in itertools.product(*[range(max(0, k + m - n), min(k, m) + 1) for m, k, n in ms]):
            yield [(a, m, k, n) for a, (m, k, n) in zip(As, ms)]


def random_problem(rng, strata, nmax):
    out = []
    for _ in range(strata):
        n = rng.randint(0, nmax)
        k, m = rng.randint(0, n), rng.randint(0, n)
        out.append((rng.randint(max(0, k + m - n), min(k, m)), m, k, n))
    return out


def test_u_orders_the_counts_like_the_exact_rule_on_every_small_problem():
    stats = {"region": 0}
    pairs = sum(check_problem(tabs, stats) for S in (1, 2) for tabs in small_problems(S, 5))
    assert pairs > 30_000 and stats["region"] > 5_000


def test_u_orders_the_counts_like_the_exact_rule_on_random_problems():
    rng = random.Random(11)
    stats = {"region": 0}
    pairs = sum(check_problem(random_problem(rng, rng.randint(1, 6), rng.choice([4, 6, 12, 40, 300])), stats)
                for _ in range(20_000))
    assert pairs > 100_000 and stats["region"] > 20_000


def test_the_snap_decides_an_exact_tie():
    """E = 6, A = 5: x = 7 is exactly as extreme.  The fp64 sum E2 misses 12 by an ulp or so; without step 2 the two
    distances differ in the last bits and x = 7 falls on the wrong side."""
    r = S10.cmh(SNAP_CASE)
    A, E, _V = S10.exact(SNAP_CASE)
    assert (A, E) == (5, 6) and r["e2"] != 12.0 and abs(r["e2"] - 12.0) < 1e-12
    lo, hi = S11.support(SNAP_CASE)
    assert lo <= SNAP_X <= hi and S11.exact_cc_extreme(SNAP_CASE, SNAP_X)
    assert S11.snap(r["e2"]) == 12.0
    assert S11.u_entry(SNAP_X, r["e2"], r["var"]) == S11.u_entry(A, r["e2"], r["var"])

    def unsnapped(x):
        delta = abs(float(x) - 0.5 * r["e2"])
        y = min(0.5, delta)
        return 1.0 / (1.0 + ((delta - y) * (delta - y)) / r["var"])
    assert unsnapped(SNAP_X) > unsnapped(A)                  # the failure step 2 is there for
    stats = {"region": 0}
    check_problem(SNAP_CASE, stats)
    # a value that is no integer is left alone, also one just outside tau
    assert S11.snap(11.5) == 11.5 and S11.snap(12.0 + 2e-6) == 12.0 + 2e-6 and S11.snap(12.0 - 5e-7) == 12.0


def test_support_is_the_range_of_the_pooled_count_by_brute_force():
    """All within-stratum labelings of problems with at most 10 isolates: the pooled counts that occur are exactly
    lo, lo + 1, ..., hi."""
    rng = random.Random(10)
    seen_wide = 0
    problems = [random_problem(rng, rng.randint(1, 4), rng.choice([2, 3, 5])) for _ in range(600)]
    problems += [[(0, 3, 2, 5), (0, 0, 0, 0), (1, 1, 1, 1), (2, 4, 3, 4)], [(5, 5, 5, 10)], [(0, 10, 0, 10)]]
    # every pair of margins with n_s <= 5 (the observed count plays no part in the support)
    problems += [[(max(0, k + m - n), m, k, n) for m, k, n in ms] for ms in itertools.product(small_margins(5), repeat=2)]
    for tabs in problems:
        if sum(n for _a, _m, _k, n in tabs) > 10:
            continue
        lo, hi = S11.support(tabs)
        assert S11.labelings_range(tabs) == set(range(lo, hi + 1)), tabs
        seen_wide += hi - lo >= 3
    assert seen_wide >= 20


def test_no_informative_stratum_gives_one_entry_of_one():
    seen = 0
    for S in (1, 2):
        for tabs in small_problems(S, 4 if S == 2 else 6):
            r = S10.cmh(tabs)
            if r["var"] != 0.0:
                continue
            lo, row, A = S11.table(tabs)
            assert row.tolist() == [1.0] and lo == A, tabs
            seen += 1
    assert seen > 1000
    # a statistic below 2^-53 rounds to u = 1.0 too (conservative: such a gene takes r = P)
    assert S11.u_entry(10, 19.0 + 2e-6, 1e12) == 1.0 and S11.u_entry(10, 15.0, 1e12) < 1.0


def test_csr_layout_and_the_reference_passes():
    """The numpy side the GPU tests compare with, on a problem small enough to follow by hand."""
    a = np.array([[[1, 0], [2, 1]]])                         # [T = 1, G = 2, S = 2]
    m = np.array([[[2, 1], [3, 1]]])
    k, n = np.array([[2, 1]]), np.array([[4, 2]])
    lo, off, tab, A = S11.csr(a, m, k, n)
    assert lo.tolist() == [[0, 1]] and off.tolist() == [0, 4, 7] and A.tolist() == [[1, 3]]
    u_obs = S11.observed(lo, off, tab, A)
    assert u_obs[0, 0] == tab[1] and u_obs[0, 1] == tab[4 + 2]
    a_perm = np.array([[0, 1], [3, 3], [1, 2]])
    u_perm = S11.permuted(lo, off, tab, 0, a_perm)
    assert u_perm[1, 0] == tab[3] and u_perm[2, 1] == tab[4 + 1]
    minu, r = S11.single_step(u_perm, u_obs[0])
    r_sd, q0 = S11.step_down(u_perm, u_obs[0])
    assert np.array_equal(q0, minu) and (r_sd <= r).all() and r_sd[np.argmin(u_obs[0])] == r[np.argmin(u_obs[0])]
