"""The restatement of spec S21 (gcmh_spec.py) held to its references on the CPU: the rational Q and rank, numpy's
pseudo-inverse of the full covariance, the chi-square of spec S20 at one stratum, the CMH statistic of spec S10 at two
classes, the choice of the dropped class, every rank-deficient family, the measured pivot threshold and exceedance
band, and the law of the shuffle.

The exhaustive part of the exceedance check: every margin set (n_sk, m_s) of K <= 3 is 461 strata with n_s <= 6, so
16 million unordered triples of them -- out of reach of rational arithmetic in a test.  Enumerated in full: one stratum
with n_s <= 6, two strata with n_s <= 4, three strata with n_s <= 2; beyond that 20 000 random margin sets of one to
three strata with n_s <= 6, and 20 000 random problems of up to 5 strata and 6 classes."""
import itertools
import random
from fractions import Fraction

import numpy as np
import pytest

import categorical_spec as cs
import cmh_spec
import gcmh_spec as gs


def _problem(rng, S, K, nmax, confine=False):
    nsk = []
    for _ in range(S):
        row = [0] * 8
        ks = rng.sample(range(K), rng.randint(1, max(1, K // 2))) if confine else range(K)
        for k in ks:
            row[k] = rng.randint(0, nmax)
        nsk.append(row)
    return [rng.randint(0, sum(r)) for r in nsk], nsk


def _a_table(rng, ms, nsk):
    """A pooled table that the margins allow: m_s isolates of stratum s drawn without replacement."""
    a = [0] * 8
    for m, row in zip(ms, nsk):
        for k in rng.sample([k for k in range(8) for _ in range(row[k])], m):
            a[k] += 1
    return a


def _corpus():
    rng = random.Random(20210)
    out = [_problem(rng, rng.randint(1, 5), rng.randint(1, 6), 12, confine=i % 2 == 0) for i in range(3000)]
    return rng, out


def _groups(ms, nsk):
    """present classes - the groups of classes that share an informative stratum (classes met in none: no contrast)."""
    parent = list(range(8))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    seen = set()
    for m, row in zip(ms, nsk):
        n = sum(row)
        if n >= 2 and 0 < m < n:
            ks = [k for k in range(8) if row[k]]
            seen.update(ks)
            for k in ks[1:]:
                parent[find(k)] = find(ks[0])
    return len(seen) - len({find(k) for k in seen})


def test_float_route_against_the_rationals_the_rank_and_the_dropped_class():
    rng, corpus = _corpus()
    worst = 0.0
    for ms, nsk in corpus:
        a = _a_table(rng, ms, nsk)
        st = gs.statistic(a, ms, nsk)
        q, rank, _rel = gs.q_exact(a, ms, nsk)
        assert st["df"] == rank == _groups(ms, nsk), (ms, nsk)
        if q:
            worst = max(worst, abs(Fraction(st["q"]) - q) / q)
        else:
            assert st["q"] <= 1e-20
        last = gs.klast(nsk) - 1
        for drop in list(range(last + 1)) + [-1]:            # any class left out, and none: the full K x K form
            assert gs.q_exact(a, ms, nsk, drop)[:2] == (q, rank), (ms, nsk, drop)
        assert (st["df"] == 0) == (not st["testable"]) and (st["df"] > 0 or (st["q"], st["p"], st["thr"]) == (0.0, 1.0, 0.0))
    print("largest relative error of the fp64 Q against the rational one: %.3g" % float(worst))
    assert worst < gs.TAU / 100


def test_float_route_against_the_pseudo_inverse_of_the_full_covariance():
    rng, corpus = _corpus()
    for ms, nsk in corpus[:1500]:
        a = _a_table(rng, ms, nsk)
        q = gs.statistic(a, ms, nsk)["q"]
        assert abs(gs.q_pinv(a, ms, nsk) - q) <= 1e-9 * max(q, 1e-9), (ms, nsk, a)


def test_one_stratum_is_the_chi_square_of_spec_s20_times_n_minus_1_over_n():
    rng = random.Random(3)
    for _ in range(400):
        ms, nsk = _problem(rng, 1, rng.randint(2, 8), 15)
        a, nk, n = _a_table(rng, ms, nsk), nsk[0], sum(nsk[0])
        if not cs.testable(a, nk):
            continue
        q, rank, _rel = gs.q_exact(a, ms, nsk)
        assert q == cs.x2_exact(a, nk) * Fraction(n - 1, n) and rank == sum(1 for x in nk if x) - 1
        x2 = cs.statistic(a, nk)[1]
        assert abs(gs.statistic(a, ms, nsk)["q"] - x2 * (n - 1) / n) <= 1e-12 * x2


def test_two_classes_are_the_cmh_statistic_of_spec_s10_without_its_correction():
    rng = random.Random(4)
    seen = 0
    for _ in range(400):
        ms, nsk = _problem(rng, rng.randint(1, 6), 2, 20)
        tables, a = [], [0] * 8
        for m, row in zip(ms, nsk):
            x = _a_table(rng, [m], [row])
            a = [p + q for p, q in zip(a, x)]
            tables.append((x[0], m, row[0], sum(row)))
        ref = cmh_spec.cmh(tables)
        st = gs.statistic(a, ms, nsk)
        if ref["var"] == 0.0:
            assert st["df"] == 0
            continue
        want = (a[0] - ref["e2"] / 2.0) ** 2 / ref["var"]
        assert st["df"] == 1 and abs(st["q"] - want) <= 1e-12 * max(want, 1.0)
        seen += 1
    assert seen > 200


FAMILIES = {
    # classes confined to disjoint strata: {1, 2} in stratum 0, {3, 4} in stratum 1 -> rank 2
    "disjoint": ([3, 2], [[5, 4, 0, 0, 0, 0, 0, 0], [0, 0, 3, 6, 0, 0, 0, 0]], 2),
    # the same two groups joined by one stratum that holds classes 2 and 3 -> rank 3
    "joined": ([3, 2, 1], [[5, 4, 0, 0, 0, 0, 0, 0], [0, 0, 3, 6, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0, 0, 0]], 3),
    # class 3 is present only where the gene is uninformative (m_s = 0 and m_s = n_s) -> it adds no contrast
    "uninformative": ([2, 0, 4], [[3, 3, 0, 0, 0, 0, 0, 0], [1, 0, 2, 0, 0, 0, 0, 0], [0, 1, 3, 0, 0, 0, 0, 0]], 1),
    # strata of one isolate add nothing
    "singletons": ([1, 0, 1, 2], [[1, 0, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0],
                                  [2, 1, 1, 0, 0, 0, 0, 0]], 2),
    # nothing informative at all: untestable
    "none": ([0, 3], [[2, 2, 0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0, 0]], 0),
    # an empty class between present ones drops out by its zero pivot
    "gap": ([2, 3], [[3, 0, 2, 0, 0, 0, 0, 2], [2, 0, 3, 0, 0, 0, 0, 1]], 2),
}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_rank_deficient_families(name):
    ms, nsk, rank = FAMILIES[name]
    rng = random.Random(len(name))
    for _ in range(20):
        a = _a_table(rng, ms, nsk)
        st = gs.statistic(a, ms, nsk)
        q, r, _rel = gs.q_exact(a, ms, nsk)
        assert st["df"] == r == rank == _groups(ms, nsk)
        assert abs(Fraction(st["q"]) - q) <= Fraction(1, 10 ** 12) * max(q, 1)
        if rank == 0:
            assert st["form"][7:] == [0.0] * 28 and (st["q"], st["thr"], st["p"]) == (0.0, 0.0, 1.0)


def _pivot_corpus():
    """(ms, nsk) with pivots that are exactly zero or small: the random corpus, 1024 strata, n_s up to 16 319, and a
    tiny stratum that alone links two groups of classes beside huge ones."""
    rng, out = _corpus()
    out = out[:1500]
    out += [_problem(rng, 1024, rng.randint(2, 8), 15, confine=i % 2 == 0) for i in range(4)]
    for i in range(8):                                   # eight classes in four disjoint pairs over 1024 strata
        nsk = []
        for _ in range(1024):
            row, g = [0] * 8, rng.randrange(4)
            row[2 * g], row[2 * g + 1] = rng.randint(0, 8), rng.randint(0, 8)
            nsk.append(row)
        out.append(([rng.randint(0, sum(r)) for r in nsk], nsk))
    for big, K in itertools.product((16319, 9000), (2, 3, 8)):
        row = [big // K if k < K else 0 for k in range(8)]
        row[0] += big - sum(row)
        for tiny in ([1] + [0] * 7, [1, 1] + [0] * 6):
            for m0, m1 in itertools.product((1, big // 2, big - 1), range(sum(tiny) + 1)):
                out.append(([m0, m1], [row, tiny]))
    for big, tiny, split in itertools.product((8158, 4000), ((1, 1), (1, 2), (3, 1)), (2, 10)):
        nsk = [[big // split, big - big // split, 0, 0, 0, 0, 0, 0],
               [0, 0, big // split, big - big // split - sum(tiny), 0, 0, 0, 0], [0, tiny[0], tiny[1], 0, 0, 0, 0, 0]]
        for m0, m1, m2 in itertools.product((1, 7, big // 2, big - 1), (0, 1, big // 5), range(sum(tiny) + 1)):
            out.append(([m0, m1, m2], nsk))
    return out


def test_theta_is_the_measured_gap_between_zero_and_nonzero_pivots():
    zero, nonzero = 0.0, 1.0
    for ms, nsk in _pivot_corpus():
        nc = max(gs.klast(nsk) - 1, 0)
        trace = []
        gs.factor(*gs.moments(ms, nsk), nc, trace=trace)
        _E, V = gs.moments_exact(ms, nsk, range(nc))
        rel = gs.factor_exact(V)[2]
        for (p, vjj), r in zip(trace, rel):
            if r is None:
                assert (p, vjj) == (0.0, 0.0)
            elif r == 0:
                zero = max(zero, abs(p) / vjj)
            else:
                nonzero = min(nonzero, float(r))
    print("largest fp64 relative pivot at an exactly zero pivot %.3g, smallest exact nonzero relative pivot %.3g"
          % (zero, nonzero))
    assert 0.0 < zero and zero * 1e4 <= gs.THETA <= nonzero / 1e4
    assert gs.THETA == 10.0 ** round(np.log10(np.sqrt(zero * nonzero)))


def _tables_of(ms, nsk):
    """Every pooled table a (a tuple of 8) that the margins allow."""
    pooled = {(0,) * 8}
    for m, row in zip(ms, nsk):
        ks = [k for k in range(8) if row[k]]
        per = set()
        for pick in itertools.product(*(range(min(row[k], m) + 1) for k in ks)):
            if sum(pick) == m:
                x = [0] * 8
                for k, v in zip(ks, pick):
                    x[k] = v
                per.add(tuple(x))
        pooled = {tuple(p + q for p, q in zip(a, b)) for a in pooled for b in per}
    return sorted(pooled)


def _check_exceedance(ms, nsk, tables, stats):
    """The fp64 rule Q_pi >= Q_obs (1 - tau) against the rational rule Q_pi >= Q_obs over all pairs of ``tables``."""
    nc = max(gs.klast(nsk) - 1, 0)
    form, _df = gs.factor(*gs.moments(ms, nsk), nc)
    E, V = gs.moments_exact(ms, nsk, range(nc))
    L, piv, _rel = gs.factor_exact(V)
    qf = [gs.q_of(a, form) for a in tables]
    qr = [gs.q_factored_exact([a[k] - E[k] for k in range(nc)], L, piv)[0] for a in tables]
    for f, r in zip(qf, qr):
        if r:
            stats["err"] = max(stats["err"], float(abs(Fraction(f) - r) / r))
    band = Fraction(gs.TAU) * Fraction(1001, 1000)      # tau and the rounding of the two fp64 values
    for obs in range(len(tables)):
        thr = qf[obs] * gs.ONE_MINUS_TAU
        for pi in range(len(tables)):
            fp, exact = qf[pi] >= thr, qr[pi] >= qr[obs]
            stats["pairs"] += 1
            if exact:
                assert fp, (ms, nsk, tables[obs], tables[pi])                   # a superset: no exact tie is lost
                stats["ties"] += pi != obs and qr[pi] == qr[obs]
            elif fp:
                assert qr[obs] - qr[pi] <= band * qr[obs], (ms, nsk, tables[obs], tables[pi])
                stats["band"] += 1


def _strata(nmax):
    out = []
    for n in range(1, nmax + 1):
        for n1 in range(n + 1):
            for n2 in range(n - n1 + 1):
                out += [(m, [n1, n2, n - n1 - n2, 0, 0, 0, 0, 0]) for m in range(n + 1)]
    return out


def test_exceedance_rule_on_the_small_margin_sets_and_on_random_problems():
    stats = dict(err=0.0, pairs=0, ties=0, band=0)
    sets = [[s] for s in _strata(6)]
    sets += [list(c) for c in itertools.combinations_with_replacement(_strata(4), 2)]
    sets += [list(c) for c in itertools.combinations_with_replacement(_strata(2), 3)]
    assert len(_strata(6)) == 461 and len(sets) == 461 + 139 * 140 // 2 + 24 * 25 * 26 // 6
    rng = random.Random(66)
    six = _strata(6)
    sets += [[rng.choice(six) for _ in range(rng.randint(1, 3))] for _ in range(20000)]
    for strata in sets:
        ms, nsk = [m for m, _row in strata], [row for _m, row in strata]
        tables = _tables_of(ms, nsk)
        if len(tables) > 12:                              # the pairs of a random dozen of them
            tables = rng.sample(tables, 12)
        _check_exceedance(ms, nsk, tables, stats)
    small = dict(stats)
    for _ in range(20000):
        ms, nsk = _problem(rng, rng.randint(1, 5), rng.randint(2, 6), 10, confine=rng.random() < 0.5)
        _check_exceedance(ms, nsk, [tuple(_a_table(rng, ms, nsk)) for _ in range(4)], stats)
    print("margin sets: %(pairs)d pairs, %(ties)d exact ties between distinct tables, %(band)d inside the band" % small)
    print("all: %(pairs)d pairs, %(ties)d ties, %(band)d inside the band, largest relative error of Q %(err).3g" % stats)
    assert small["ties"] > 1000 and stats["err"] < gs.TAU / 100


def test_many_genes_at_once_are_the_scalar_route_bit_for_bit():
    rng = random.Random(9)
    for S, K in ((1, 3), (4, 8), (7, 5)):
        _ms, nsk = _problem(rng, S, K, 9, confine=S == 7)
        ms = [[rng.randint(0, sum(r)) for r in nsk] for _ in range(40)]
        a = [_a_table(rng, m, nsk) for m in ms]
        nc = max(gs.klast(nsk) - 1, 0)
        E, V = gs.moments_many(np.array(ms), nsk)
        form, df = gs.factor_many(E, V, nc)
        q = gs.q_many(np.array(a), form)
        for g in range(40):
            st = gs.statistic(a[g], ms[g], nsk)
            assert E[g].tolist() == st["E"] and form[g].tolist() == st["form"] and df[g] == st["df"] and q[g] == st["q"]


def test_the_shuffle_keeps_the_class_multiset_of_every_stratum():
    rng = random.Random(12)
    N, S = 57, 4
    strata = [rng.randrange(S) for _ in range(N)]
    codes = [rng.randrange(0, 4) for _ in range(N)]
    assert gs.lrow(codes, strata, S) == [codes[i] for s in range(S) for i in range(N) if strata[i] == s and codes[i]]
    rows = [gs.perm_row(77, 1, pi, codes, strata, S) for pi in range(30)]
    assert len({tuple(r) for r in rows}) > 25
    for row in rows:
        assert [c == 0 for c in row] == [c == 0 for c in codes]
        assert gs.margins(row, strata, S) == gs.margins(codes, strata, S)
    one = [0] * N                                           # one stratum: S20's rows at the same seed
    assert [gs.perm_row(77, 1, pi, codes, one, 1) for pi in range(5)] == [cs.perm_row(77, 1, pi, codes) for pi in range(5)]


def test_the_clonal_scenario_meets_its_bars_in_the_restatement_alone():
    genes, labels, strata = gs.clonal_scenario()
    classes, codes = cs.codes_of(labels)
    nk, nsk = cs.sizes(codes, 3), gs.margins(codes, strata, 2)
    chi, gcmh = [], []
    for gene in genes:
        a, ms = gs.counts(gene, codes, strata, 2)
        chi.append(cs.statistic(a[:3], nk)[3])
        gcmh.append(gs.statistic(a, ms, nsk)["p"])
    assert chi[0] < 1e-6 and gcmh[0] > 0.05            # the lineage marker: tiny pooled, unremarkable within
    assert gcmh[1] < 1e-3                              # the gene that follows the label inside the lineages
    assert chi[2] > 0.05 and gcmh[2] > 0.05


def test_the_kernels_are_built_with_the_measured_constants():
    import os
    import re
    import __graft_entry__ as ge
    from scoary_amd import engine
    with open(os.path.join(os.path.dirname(ge.HIP_SRCS[0]), "scoary_gcmh.hip")) as f:
        text = f.read()
    assert float(re.search(r"kGcmhTheta = ([0-9.e-]+);", text).group(1)) == gs.THETA
    assert float(re.search(r"kGcmhTau = ([0-9.e-]+);", text).group(1)) == gs.TAU == cmh_spec.TAU
    assert engine.GCMH_FORM == gs.FORM == 35 and engine.CATEGORICAL_MAX_CLASSES == gs.MAX_CLASSES
