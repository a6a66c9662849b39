"""Spec S10 on the CPU: the plain-Python restatement (tests/cmh_spec.py) against a published anchor, and its
rejection region against the exact rule in rational arithmetic."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import cmh_cases as C
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


# -- the constructed cases of tests/cmh_cases.py reach what the GPU tests (test_gpu_cmh_limits.py) hold the kernel to --

def _edge_tables():
    genes, traits, strata, names = C.edge_case()
    a, m, k, n = C.recount(genes, traits, strata, len(C.EDGE_NK))
    assert [(int(n[0, s]), int(k[0, s])) for s in range(len(C.EDGE_NK))] == list(C.EDGE_NK)
    for g, name in enumerate(names):                 # the expansion to isolates gives back the (a, m) it was given
        assert [(int(a[0, g, s]), int(m[0, g, s])) for s in range(len(C.EDGE_NK))] == list(C.EDGE_GENES[name])
    return a, m, k, n, names


def test_the_edge_case_meets_every_condition_it_is_built_for():
    a, m, k, n, names = _edge_tables()
    G = a.shape[1]
    tabs = {name: C.tables(a, m, k, n, 0, g) for g, name in enumerate(names)}
    res = {name: S.cmh(t) for name, t in tabs.items()}
    K = sum(kk for _n, kk in C.EDGE_NK)
    # no informative stratum
    assert res["dead"]["var"] == 0.0 and res["none"]["var"] == 0.0 and res["all"]["var"] == 0.0
    # A = E: the middle branch of the region
    r = res["a_equals_e"]
    assert r["var"] > 0 and abs(2.0 * r["a"] - r["e2"]) <= S.TAU and r["crit"] == (0, 0) and r["stat"] == 0.0
    assert S.exact(tabs["a_equals_e"])[0] == S.exact(tabs["a_equals_e"])[1]
    # half a count from E: inside the continuity correction, outside the middle branch
    r = res["inside_cc"]
    A, E, _V = S.exact(tabs["inside_cc"])
    assert abs(A - E) == Fraction(1, 2) and r["stat"] == 0.0 and r["var"] > 0 and abs(2.0 * r["a"] - r["e2"]) > S.TAU
    # lo of S10 below 0 before the clamp: A > 2E + 1
    r = res["lo_clamp"]
    A, E, _V = S.exact(tabs["lo_clamp"])
    assert A > 2 * E + 1 and math.floor((r["e2"] - float(r["a"])) + S.TAU) + 1 < 0
    assert r["crit"][0] == 0 and r["crit"][1] == r["a"] > 0              # base == 0 with span > 0: accepts 0 .. A - 1
    # hi of S10 above K before the clamp: 2E - A > K
    r = res["hi_clamp"]
    A, E, _V = S.exact(tabs["hi_clamp"])
    assert 2 * E - A > K and math.ceil((r["e2"] - float(r["a"])) - S.TAU) - 1 > K
    assert r["crit"] == (A + 1, K - A) and r["crit"][0] + r["crit"][1] == K + 1
    # an exact tie: the mirror image of A is an integer of the support, and extreme
    r = res["mirror_tie"]
    A, E, _V = S.exact(tabs["mirror_tie"])
    mirror = 2 * E - A
    lo, hi = S.support(tabs["mirror_tie"])
    assert mirror.denominator == 1 and mirror != A and lo <= mirror <= hi
    assert S.in_region(r["crit"], int(mirror)) and S.in_region(r["crit"], A)
    assert not S.in_region(r["crit"], int(E)) and r["crit"][1] == abs(int(mirror) - A) - 1
    # odds = inf: no discordant pair of one kind
    assert res["odds_inf"]["odds"] == math.inf and res["odds_inf"]["var"] > 0
    assert math.isnan(res["none"]["odds"])
    # the second trait: strata with n = 0 and n = 1 that the mask made
    assert [int(x) for x in n[1, [0, 3, 7]]] == [1, 0, 0] and (n[0] > 0).all()
    live = sum(S.cmh(C.tables(a, m, k, n, 1, g))["var"] > 0 for g in range(G))
    assert 0 < live < G
    # region and exact rule agree on the whole support of every gene of both traits
    for t in range(2):
        for g in range(G):
            tb = C.tables(a, m, k, n, t, g)
            lo, hi = S.support(tb)
            assert C.exact_rule_mismatches(tb, S.cmh(tb)["crit"], range(lo, hi + 1)) == []


def test_the_graded_case_has_tiny_subnormal_and_zero_p():
    genes, traits, strata = C.graded_case()
    want = C.restate(*C.recount(genes, traits, strata, 4))
    stat, p = want["stat"][0], want["p"][0]
    assert stat.min() < 70 and stat.max() > 1500 and (want["var"] > 0).all()
    assert ((p >= C.P_NORMAL) & (p < 1e-200)).sum() >= 3                 # normal doubles below 1e-200
    assert ((p > 0) & (p < 2.2250738585072014e-308)).sum() >= 1          # subnormals
    assert ((p == 0.0) & (stat > 1400)).sum() >= 1                       # underflow to an exact zero
    assert (p > 1e-30).sum() >= 3
    print("graded case: stat %.1f .. %.1f, %d subnormal p, %d zero p"
          % (stat.min(), stat.max(), ((p > 0) & (p < 2.2250738585072014e-308)).sum(), (p == 0).sum()))


@pytest.mark.parametrize("name", list(C.BATCH_CASES))
def test_the_batch_cases_regions_equal_the_exact_rule_on_the_whole_support(name):
    """The counts a permutation can reach are those of the support: on all of them the restatement's region is the
    exact rule, up to the stated slack at a near tie."""
    genes, traits, strata, Sn, _P, _batch, _tw = C.batch_case(name)
    a, m, k, n = C.recount(genes, traits, strata, Sn)
    informative = 0
    for t, g in C.subsample_pairs(traits.shape[0], genes.shape[0]):
        tb = C.tables(a, m, k, n, t, g)
        r = S.cmh(tb)
        lo, hi = S.support(tb)
        assert C.exact_rule_mismatches(tb, r["crit"], range(lo, hi + 1)) == [], (name, t, g)
        informative += r["crit"][1] > 0
    assert informative >= 10


def test_the_limit_layouts_are_what_they_claim():
    N, Sn = C.LIMIT_N, C.LIMIT_S
    word = np.arange(N) // 32
    assert word.max() == 639 and N == 20479 and Sn == 1024
    segments = {}
    for name in C.LIMIT_GENES:
        st = C.limit_strata(name)
        assert st.shape == (N,) and st.min() >= 0 and st.max() == Sn - 1 - (name == "blocked")
        segments[name] = len(np.unique(st * 1024 + word))
        # stratum indices and word indices past 8 bits together, in every layout
        assert ((st >= 256) & (word >= 256)).any()
    # interleaved: no two members of a stratum share a word, so there are N segments, as many as the scratch holds
    assert segments["interleaved"] == N
    # blocked: contiguous, blocks of one, of more than 32 and more than 64 members, indices without a member
    st = C.limit_strata("blocked")
    sizes = np.bincount(st, minlength=Sn)
    assert (np.diff(st) >= 0).all()
    assert (sizes == 1).sum() >= 20 and ((sizes > 32) & (sizes <= 64)).sum() >= 5 and (sizes > 64).sum() >= 5
    assert sizes[0] == 0 and sizes[512] == 0 and sizes[Sn - 1] == 0
    assert (sizes[1:512] > 0).any() and (sizes[513:] > 0).any()
    assert (np.flatnonzero(np.diff(st)) % 32 != 31).sum() > 500          # boundaries inside words
    _genes, traits, _st = C.limit_case("blocked")
    assert sizes[7] > 0 and (traits[1, st == 7] == 2).all() and (traits[0, st == 7] != 2).all()
    # two_level: several members of a stratum per word, not adjacent; runs longer than a word cannot occur, runs
    # of up to 16 members start at every offset of the segment builder's 20-member chunks
    st = C.limit_strata("two_level")
    order = np.argsort(st, kind="stable")
    key = st[order] * 1024 + word[order]
    heads = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    runs = np.diff(np.r_[heads, N])
    assert segments["two_level"] < N // 8 and runs.max() == 16 and (runs >= 10).sum() > 1000
    per = -(-N // 1024)
    assert per == 20 and ((heads % per) + runs > per).sum() > 300        # runs that cross a chunk end
    for name in C.LIMIT_GENES:
        _g, traits, _s = C.limit_case(name)
        assert traits.shape == (C.LIMIT_T, N) and (traits == 2).any(1).sum() >= 2
    assert max(C.LIMIT_GENES.values()) > 256 and max(C.LIMIT_GENES.values()) % 256
