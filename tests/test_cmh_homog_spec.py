"""Spec S14 on the CPU: the restatement (cmh_homog_spec.py) against the UCBAdmissions anchor, against the same
functional at 80 digits, its chi-square tail against mpmath (and SciPy where it imports), the laws of the statistic
and the branches the edge genes of the device test are there to reach."""
import itertools
import math
import random
from decimal import Decimal

import numpy as np
import pytest

import cmh_cases as C
import cmh_homog_spec as S14
import cmh_spec as S10

DFS = (1, 2, 3, 4, 5, 9, 10, 49, 50, 255, 256, 511, 1022, 1023)


def rel(got, want):
    return abs(got - want) / abs(want)


def ucb_tables():
    return S10.tables_abcd(S10.UCB.values())


# ---- 1. the anchor ----------------------------------------------------------------------------------------------
def test_ucb_admissions_anchor():
    tabs, want = ucb_tables(), S14.UCB_ANCHOR
    psi = S10.cmh(tabs)["odds"]
    bd, tarone, df, p = S14.homogeneity(tabs, psi)
    print("UCB: psi %r bd %r tarone %r df %d p %r" % (psi, bd, tarone, df, p))
    assert rel(psi, want["psi"]) <= 1e-12 and rel(bd, want["bd"]) <= 1e-12 and rel(tarone, want["tarone"]) <= 1e-12
    assert df == want["df"] == 5 and rel(p, want["p"]) <= 1e-12
    assert rel(S14.chi2_sf(bd, df), 0.0020713903) <= 1e-7                    # the uncorrected p, to its printed digits
    # R: BreslowDayTest(UCBAdmissions, correct = TRUE): X-squared = 18.826, df = 5, p-value = 0.002071
    assert round(tarone, 3) == 18.826 and float("%.4g" % p) == 0.002071


# ---- 2. the restatement against 80 digits -----------------------------------------------------------------------
def _errors(tabs, psi):
    """(relative error of bd, error of Tarone's: relative or, where smaller, absolute) of the restatement; the checks
    every defined problem has to pass."""
    trace = []
    bd, tarone, df, p = S14.homogeneity(tabs, psi, trace)
    want = S14.exact(tabs, psi)
    if want is None:
        assert (df, p) == (0, 1.0) and math.isnan(bd) and math.isnan(tarone)
        return None
    bd_x, tarone_x, df_x = want
    assert df == df_x == len(trace) - 1
    assert math.isfinite(bd) and math.isfinite(tarone) and bd >= 0.0 and 0.0 <= p <= 1.0, (tabs, psi, bd, tarone)
    for _branch, x, (lo, hi) in trace:                                       # the sign rule's root is the support's
        assert lo <= x <= hi, (tabs, psi, x, lo, hi)
    bd_d, tarone_d = Decimal(bd), Decimal(tarone)                              # (a double is a Decimal exactly)
    e_bd = float(abs(bd_d - bd_x) / bd_x) if bd_x else abs(bd)
    clamped = max(tarone_x, Decimal(0))
    e_abs = float(abs(tarone_d - clamped))
    e_t = min(float(abs(tarone_d - clamped) / clamped), e_abs) if clamped else e_abs
    assert e_bd <= 1e-8 and (e_t <= 1e-8 or e_abs <= 1e-12), (tabs, psi, bd, float(bd_x), tarone, float(tarone_x))
    return e_bd, e_t


def _stratum_tables(nmax):
    return [(a, m, k, n) for n in range(1, nmax + 1) for k in range(n + 1) for m in range(n + 1)
            for a in range(max(0, k + m - n), min(k, m) + 1)]


def test_every_pair_of_small_strata_against_80_digits():
    one = _stratum_tables(5)
    worst, defined = 0.0, 0
    for tabs in itertools.product(one, one):
        psi = S10.cmh(list(tabs))["odds"]
        e = _errors(list(tabs), psi)
        if e is not None:
            defined += 1
            worst = max(worst, *e)
    print("S14 restatement, every pair of strata with n <= 5: %d pairs, %d defined, worst error %.3e"
          % (len(one) ** 2, defined, worst))
    assert defined > 1000


def _random_problem(rng, mode):
    """mode 0: ordinary (n <= 300); 1: mixed sizes; 2: mixed sizes with margins forced toward a = min(k, m)."""
    tabs = []
    for _s in range(rng.randint(2, 10)):
        n = rng.choice([2, 3, 5, 40, 300, 3000]) if mode else rng.randint(2, 300)
        if mode == 2:
            k = rng.randint(1, n - 1)
            m = k if rng.random() < 0.7 else rng.randint(1, n - 1)
            lo, hi = max(0, k + m - n), min(k, m)
            a = hi if rng.random() < 0.8 else rng.randint(lo, hi)
        else:
            k, m = rng.randint(0, n), rng.randint(0, n)
            a = rng.randint(max(0, k + m - n), min(k, m))
        tabs.append((a, m, k, n))
    return tabs


def test_random_problems_against_80_digits():
    worst, worst_psi, defined, count = [0.0, 0.0, 0.0], 0.0, [0, 0, 0], 0
    for mode in (0, 1, 2):
        rng = random.Random(14 + mode)
        for _i in range(1334 if mode < 2 else 1332):
            tabs = _random_problem(rng, mode)
            count += 1
            psi = S10.cmh(tabs)["odds"]
            e = _errors(tabs, psi)
            if e is not None:
                defined[mode] += 1
                worst[mode] = max(worst[mode], *e)
                worst_psi = max(worst_psi, psi)
    print("S14 restatement, %d random problems (%s defined): worst error ordinary %.3e, mixed sizes %.3e, forced "
          "margins %.3e; psi up to %.3g" % (count, defined, worst[0], worst[1], worst[2], worst_psi))
    assert count == 4000 and min(defined) > 500 and worst_psi > 1e3


# ---- 3. the tail ------------------------------------------------------------------------------------------------
def _grid(df):
    lo, hi = df * 1e-2, min(df * 370.0, 1400.0)
    steps = 60
    return [lo * (hi / lo) ** (i / steps) for i in range(steps + 1)] + [float(df)]


def test_chi2_sf_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    try:
        from scipy.special import chdtrc
    except ImportError:
        chdtrc = None
    worst, worst_scipy, checked = (0.0, None), 0.0, 0
    for df in DFS:
        for x in _grid(df):
            want = mp.gammainc(mp.mpf(df) / 2, mp.mpf(x) / 2, mp.inf, regularized=True)
            got = S14.chi2_sf(x, df)
            assert 0.0 <= got <= 1.0
            if want < 1e-290:
                assert got <= 1e-290, (df, x, got)
                continue
            checked += 1
            r = float(abs(got - want) / want)
            if r > worst[0]:
                worst = (r, (df, x))
            if chdtrc is not None:
                ref = float(chdtrc(df, x))
                worst_scipy = max(worst_scipy, abs(got - ref) / ref)
    print("chi2_sf against mpmath: %d points, worst relative error %.3e at (df, x) = %s; against scipy.special.chdtrc "
          "%.3e" % (checked, worst[0], worst[1], worst_scipy))
    assert checked > 500 and worst[0] <= 1e-10
    assert worst_scipy <= 1e-10                                              # (0.0 without SciPy)


def test_chi2_sf_ends():
    for df in DFS:
        assert S14.chi2_sf(0.0, df) == 1.0 and S14.chi2_sf(math.inf, df) == 0.0
        assert S14.chi2_sf(1e-300, df) == 1.0 and 0.0 <= S14.chi2_sf(1e5, df) <= 1e-290
        assert rel(S14.chi2_sf(float(df), df), S14.chi2_sf(df * (1 + 1e-13), df)) < 1e-10
    assert rel(S14.chi2_sf(2.0, 2), math.exp(-1.0)) < 1e-15 and rel(S14.chi2_sf(1.0, 1), math.erfc(math.sqrt(0.5))) < 1e-15


# ---- 4. laws ----------------------------------------------------------------------------------------------------
def test_laws_of_the_statistic():
    rng = random.Random(1973)
    seen = 0
    for i in range(600):
        tabs = _random_problem(rng, i % 3)
        psi = S10.cmh(tabs)["odds"]
        bd, tarone, df, p = S14.homogeneity(tabs, psi)
        L = sum(S14.informative(m, k, n) for _a, m, k, n in tabs)
        if not (0.0 < psi < math.inf) or L < 2:
            assert (df, p) == (0, 1.0) and math.isnan(bd) and math.isnan(tarone)
            continue
        seen += 1
        assert 0.0 <= tarone <= bd and df == L - 1 and 0.0 <= p <= 1.0
        # gene and label change roles: (a, m, k, n) -> (a, k, m, n); R and Q are the same doubles
        swapped = [(a, k, m, n) for a, m, k, n in tabs]
        assert S10.cmh(swapped)["odds"] == psi
        bd2, tarone2, df2, _p2 = S14.homogeneity(swapped, psi)
        assert df2 == df and abs(bd2 - bd) <= 1e-9 * bd
        assert abs(tarone2 - tarone) <= 1e-9 * tarone or abs(tarone2 - tarone) <= 1e-12
    assert seen > 300


def test_undefined_results():
    tabs = ucb_tables()
    for psi in (0.0, math.inf, math.nan, -1.0):
        got = S14.homogeneity(tabs, psi)
        assert got[2:] == (0, 1.0) and math.isnan(got[0]) and math.isnan(got[1])
        assert S14.exact(tabs, psi) is None
    for few in (tabs[:1], [], tabs[:1] + [(0, 0, 3, 9), (2, 2, 0, 5), (4, 9, 4, 9), (0, 1, 1, 1), (0, 0, 0, 0)]):
        got = S14.homogeneity(few, 0.9)
        assert got[2:] == (0, 1.0) and math.isnan(got[0]) and math.isnan(got[1])
    assert S14.homogeneity(tabs[:2], 0.9)[2] == 1


def test_two_strata_that_are_copies_of_each_other():
    """Both strata are fitted by the same table with the same d, so Tarone's correction takes all of the statistic:
    p = 1 exactly, always.  stat_tarone = 0 exactly where the table is its own fit in doubles (a n = k m: psi = 1.0 and
    x = a without a rounding, so d = 0) -- asserted; elsewhere d is the rounding error of x, at most a few ulp of n,
    so bd <= 16 (n 2^-50)^2, and bd = 2 fl(d d w) and fl(4 d d) / fl(2 / w) part by one rounding at the most:
    stat_tarone <= bd 2^-50, which the clamp at 0 removes in all but a few problems."""
    count = exact_zero = own_fit = 0
    for a, m, k, n in _stratum_tables(12) + [(30, 100, 90, 400), (511, 600, 825, 933), (7, 1000, 9, 3000),
                                              (250, 500, 1000, 2000)]:
        if not S14.informative(m, k, n):
            continue
        tabs = [(a, m, k, n)] * 2
        psi = S10.cmh(tabs)["odds"]
        bd, tarone, df, p = S14.homogeneity(tabs, psi)
        if df == 0:
            assert not 0.0 < psi < math.inf
            continue
        count += 1
        exact_zero += tarone == 0.0
        assert df == 1 and p == 1.0, (tabs, psi, bd, tarone, p)
        assert bd <= 16.0 * (n * 2.0 ** -50) ** 2 and tarone <= bd * 2.0 ** -50, (tabs, psi, bd, tarone)
        if a * n == k * m:
            own_fit += 1
            assert psi == 1.0 and bd == 0.0 and tarone == 0.0, (tabs, psi, bd, tarone)
    print("two copies of one stratum: %d problems, Tarone's statistic exactly 0 in %d, %d of them their own fit"
          % (count, exact_zero, own_fit))
    assert count > 300 and own_fit > 20


# ---- 5. the edge genes of the device test -----------------------------------------------------------------------
def test_edge_genes_reach_their_branches():
    genes, traits, strata, names = S14.edge_case()
    assert S14.EDGE_NK == C.EDGE_NK
    a, m, k, n = C.recount(genes, traits, strata, len(S14.EDGE_NK))
    assert n[0].tolist() == [nk[0] for nk in S14.EDGE_NK] and k[0].tolist() == [nk[1] for nk in S14.EDGE_NK]
    assert n[1, 7] == 0 and n[1, 3] == 0 and (n[1, 0], k[1, 0]) == (1, 1)     # emptied by the mask; cut to one isolate
    assert n[0, 3] == n[0, 4] == 1                                            # strata of one isolate

    def run(name, t=0):
        g = names.index(name)
        tabs = C.tables(a, m, k, n, t, g)
        psi = S10.cmh(tabs)["odds"]
        trace = []
        return tabs, psi, S14.homogeneity(tabs, psi, trace), [b for b, _x, _s in trace]

    _tabs, psi, res, br = run("psi_one")
    assert psi == 1.0 and br == ["B>=0", "B>=0"] and res[2] == 1 and res[0] > 1.0          # L = 2
    _tabs, psi, res, br = run("b_negative")
    assert psi < 1.0 and br == ["B<0", "B>=0"] and res[2] == 1 and math.isfinite(res[0])
    _tabs, psi, res, br = run("psi_above_one")
    assert 1.0 < psi < math.inf and br == ["B>=0"] * 3 and res[2] == 2
    for name, want in (("psi_zero", 0.0), ("psi_inf", math.inf)):
        tabs, psi, res, br = run(name)
        assert psi == want and sum(S14.informative(mm, kk, nn) for _a, mm, kk, nn in tabs) == 2
        assert br == [] and res[2:] == (0, 1.0) and math.isnan(res[0]) and math.isnan(res[1])
    for name in ("none", "all"):
        for t in (0, 1):
            _tabs, psi, res, br = run(name, t)
            assert math.isnan(psi) and br == [] and res[2:] == (0, 1.0) and math.isnan(res[0])
    _tabs, psi, res, br = run("one_stratum")
    assert 1.0 < psi < math.inf and br == ["B>=0"] and res[2:] == (0, 1.0) and math.isnan(res[0])      # L = 1
    tabs, psi, res, br = run("with_n_one")
    assert tabs[3] == (1, 1, 1, 1) and tabs[4] == (0, 1, 0, 1) and len(br) == 3 and res[2] == 2
    _tabs, _psi, res0, br0 = run("masked", 0)
    tabs1, _psi, res1, br1 = run("masked", 1)
    assert len(br0) == 4 and res0[2] == 3 and len(br1) == 2 and res1[2] == 1
    assert tabs1[7] == (0, 0, 0, 0) and tabs1[3] == (0, 0, 0, 0) and tabs1[0] == (1, 1, 1, 1)
