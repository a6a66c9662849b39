"""What the randomised corpora of strata_stress_cases.py reach, shown on the CPU from the draws and the references
alone: the committed seeds and case counts hold every shape, pair and count the suite is for, and HOLDS names one case
for each.  A seed or a case count that is changed has to keep this file green."""
import math

import numpy as np
import pytest

import cmh_cases as C
import cmh_exact_spec as S12
import cmh_homog_spec as S14
import cmh_spec as S10
import strata_stress_cases as ssc

# item -> (family, case) of one case that holds it (test_every_item_is_where_this_table_says)
HOLDS = {
    "S > 256": ('B', 2),
    "S > N": ('A', 0),
    "N on a word boundary": ('A', 0),
    "N one past a word boundary": ('A', 1),
    "N = 1": ('A', 2),
    "a stratum with n = 0 for one trait only": ('A', 0),
    "a trait constant inside every stratum": ('A', 2),
    "S = 1024": ('B', 5),
    "a one-point support": ('B', 0),
    "the observed count at the low end": ('B', 0),
    "the observed count at the high end": ('B', 0),
    "a support longer than 64": ('B', 2),
    "a support longer than 256": ('B', 3),
    "a support longer than 256 from N = 511 or 700 and few strata": ('B', 10),
    "an exact p below 1e-20": ('B', 1),
    "homogeneity undefined (df = 0)": ('B', 0),
    "homogeneity with df >= 255": ('B', 7),
    "word boundary, emptied strata and an end of the support together": ('B', 6),
    "exact ties that the doubles of the restatement break": ('B', 12),
}


def problems(family):
    pools = ssc.POOLS[family]
    prs = [ssc.draw(case, pools) for case in range(pools["cases"])]
    return [ssc.d_traits(pr) for pr in prs] if family == "D" else prs


def shape_items(pr):
    """The shape items of one problem."""
    items = set()
    if pr.S > 256:
        items.add("S > 256")
    if pr.S == 1024:
        items.add("S = 1024")
    if pr.S > pr.N:
        items.add("S > N")
    if pr.N in (32, 64):
        items.add("N on a word boundary")
    if pr.N in (33, 65):
        items.add("N one past a word boundary")
    if pr.N == 1:
        items.add("N = 1")
    _a, _m, _k, n = C.recount(pr.genes[:1], pr.traits, pr.strata, pr.S)
    if ((n == 0).any(axis=0) & (n > 0).any(axis=0)).any():
        items.add("a stratum with n = 0 for one trait only")
    if pr.emptied:
        items.add("strata emptied by missing values")
    if pr.constant is not None:
        items.add("a trait constant inside every stratum")
    if (pr.traits == 2).any():
        items.add("missing values")
    if pr.P % 64:
        items.add("P no multiple of 64")
    return items


def survey():
    """{(family, case): items} and family B's (pairs, near ties)."""
    found, pairs, ties = {}, 0, 0
    for family in ssc.POOLS:
        for pr in problems(family):
            found[(family, pr.case)] = shape_items(pr)
    for pr in problems("B"):
        items = found[("B", pr.case)]
        a, m, k, n = C.recount(pr.genes, pr.traits, pr.strata, pr.S)
        for t, g in ssc.b_pairs(pr):
            tabs = C.tables(a, m, k, n, t, g)
            if ssc.b_exact(pr):
                lo, tab, p, _region, tie = S12.reference(tabs)
                pairs, ties = pairs + 1, ties + bool(tie)
                _lo, W, _D = S12.exact_weights(tabs)
                f = S12.float_pmf(tabs)[1]
                if len(W) > 2 and W == W[::-1] and (f != f[::-1]).any():
                    items.add("exact ties that the doubles of the restatement break")
            else:
                lo, tab, p, _region = S12.restate(tabs)
            A, L = S10.cmh(tabs)["a"], len(tab)
            if L == 1:
                items.add("a one-point support")
                assert p == 1.0
            else:
                if A == lo:
                    items.add("the observed count at the low end")
                if A == lo + L - 1:
                    items.add("the observed count at the high end")
            if L > 64:
                items.add("a support longer than 64")
            if L > 256:
                items.add("a support longer than 256")
                if pr.N in (511, 700) and pr.S <= 3:
                    items.add("a support longer than 256 from N = 511 or 700 and few strata")
            if p < 1e-20:
                items.add("an exact p below 1e-20")
            if (n[t] == 0).sum() >= 2 and pr.N in (32, 64) and L > 1 and A in (lo, lo + L - 1):
                items.add("word boundary, emptied strata and an end of the support together")
        for t in range(pr.T):
            for g in ssc.b_genes(pr):
                tabs = C.tables(a, m, k, n, t, g)
                df = S14.homogeneity(tabs, S10.cmh(tabs)["odds"])[2]
                if df == 0:
                    items.add("homogeneity undefined (df = 0)")
                if df >= 255:
                    items.add("homogeneity with df >= 255")
    return found, pairs, ties


@pytest.fixture(scope="module")
def corpus():
    return survey()


SHAPES = ("S > 256", "S > N", "N on a word boundary", "N one past a word boundary", "N = 1",
          "a stratum with n = 0 for one trait only", "a trait constant inside every stratum")
B_ITEMS = ("S = 1024", "S > 256", "a one-point support", "the observed count at the low end",
           "the observed count at the high end", "a support longer than 64", "a support longer than 256",
           "a support longer than 256 from N = 511 or 700 and few strata", "an exact p below 1e-20",
           "homogeneity undefined (df = 0)", "homogeneity with df >= 255",
           "word boundary, emptied strata and an end of the support together",
           "exact ties that the doubles of the restatement break")


def cases_with(found, item, family=None):
    return sorted(key for key, items in found.items() if item in items and family in (None, key[0]))


def test_the_corpus_contains_the_shapes(corpus):
    found, _pairs, _ties = corpus
    for item in SHAPES:
        assert cases_with(found, item), item


def test_family_b_contains_the_pairs(corpus):
    found, _pairs, _ties = corpus
    for item in B_ITEMS:
        assert cases_with(found, item, "B"), item


def test_near_ties_stay_under_one_percent(corpus):
    _found, pairs, ties = corpus
    print("family B: %d pairs held to the Fractions, %d near ties" % (pairs, ties))
    assert pairs >= 100 and ties <= 0.01 * pairs


@pytest.mark.parametrize("family", ["C", "D", "E"])
def test_counting_families_have_missing_values_and_ragged_permutation_counts(corpus, family):
    found, _pairs, _ties = corpus
    assert cases_with(found, "missing values", family) and cases_with(found, "P no multiple of 64", family)


def test_family_e_has_wavefronts_without_slots_and_the_k_step_limit():
    prs = problems("E")
    assert any(pr.G == 33 for pr in prs) and any(pr.N == 2048 for pr in prs)
    assert all(pr.N <= 2048 for pr in prs)


def test_family_d_has_both_budgets_and_enough_genes_to_rank():
    """A step-down over one or three genes says little: half of the cases have 63 genes or more, among them one under
    each budget, one past the matrix cores' isolates and one with more strata than a block has lanes."""
    prs = [pr for pr in problems("D") if pr.G >= 63]
    assert len(prs) >= 5
    assert any(pr.case % 5 == 1 and pr.T >= 2 for pr in prs) and any(pr.case % 5 == 3 and pr.P >= 2 for pr in prs)
    assert any(pr.N >= 2047 for pr in prs) and any(pr.S > 256 and pr.N >= 300 for pr in prs)
    assert any(pr.emptied for pr in prs) and any(pr.P % 64 for pr in prs)


def test_every_item_is_where_this_table_says(corpus):
    found, _pairs, _ties = corpus
    assert set(HOLDS) >= set(SHAPES) | set(B_ITEMS)
    for item, key in HOLDS.items():
        assert item in found[key], (item, key)


def test_draws_do_not_depend_on_the_order_they_are_made_in():
    one, again = ssc.draw(3, ssc.POOLS["B"]), ssc.draw(3, ssc.POOLS["B"])
    assert np.array_equal(one.genes, again.genes) and np.array_equal(one.traits, again.traits)
    assert np.array_equal(one.strata, again.strata) and (one.seed, one.level) == (again.seed, again.level)
    assert not math.isnan(one.level)


if __name__ == "__main__":                           # the table above, as the committed seeds give it
    found, pairs, ties = survey()
    for item in sorted(set().union(*found.values())):
        print("%-70s %s" % (item, cases_with(found, item)[:6]))
    print(pairs, ties)
