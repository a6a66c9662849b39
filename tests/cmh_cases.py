"""Inputs and host-side references of the Cochran-Mantel-Haenszel tests (spec S10): deterministic, numpy only at
import (Case touches the engine it is handed, nothing else does), so the CPU tests can build the same cases and show
from the restatement (cmh_spec.py) alone that they reach the edges they are meant to reach.  A helper, not a test."""
import math
from fractions import Fraction

import numpy as np

import cmh_exact_odds_spec as S13
import cmh_exact_spec as S12
import cmh_homog_spec as S14
import cmh_spec as S10

P_NORMAL = 2.3e-308                  # just above the smallest normal double: below it p has no relative accuracy


class Case:
    """Genes, traits (0 / 1, 2 = missing) and strata as numpy arrays and on the device."""

    def __init__(self, eng, genes, traits, strata, S=None):
        from scoary_amd.engine import pack_bits_rows
        self.genes, self.traits, self.strata = genes.astype(np.uint8), traits.astype(np.uint8), np.asarray(strata)
        (self.G, self.N), self.T = genes.shape, traits.shape[0]
        self.gm = eng.pack_dense(self.genes)
        self.trv = eng.vecrows(pack_bits_rows((self.traits == 1).astype(np.uint8)), self.N)
        self.mkv = eng.vecrows(pack_bits_rows((self.traits != 2).astype(np.uint8)), self.N)
        self.sp = eng.strata_plan(self.strata, self.trv, self.mkv, self.N, S=S)
        self.S = self.sp.S

    def recount(self):
        """(a, m) int64 [T, G, S] and (k, n) int64 [T, S] with numpy."""
        return recount(self.genes, self.traits, self.strata, self.S)

    def label_rows(self, eng, P, seed):
        """The stratified label bits [T, P, N] of P permutations, downloaded from the generator."""
        plan = eng.trait_plan(self.trv, self.mkv, self.N)
        rows = eng.perm_generate(self.mkv, plan.margins, self.N, P, 0, seed, strata=self.sp).cpu().numpy()
        return np.unpackbits(rows.view(np.uint8).reshape(self.T, P, -1), axis=2, bitorder="little")[:, :, :self.N]

    def labels(self, eng, P, seed):
        """The label bits [T, P, N] and the pooled counts [T, P, G] of P permutations."""
        bits = self.label_rows(eng, P, seed)
        return bits, pooled_counts(bits, self.genes)


def pooled_counts(bits, genes):
    """popc(gene & label) of every (trait, permutation, gene), int64 [T, P, G] (float32 products of 0 / 1 summed
    over fewer than 2^24 isolates are exact)."""
    assert genes.shape[1] < 1 << 24
    return np.rint(bits.astype(np.float32) @ genes.astype(np.float32).T).astype(np.int64)


def recount(genes, traits, strata, S):
    """(a, m) int64 [T, G, S] and (k, n) int64 [T, S]: one np.bincount over the carriers of every gene."""
    strata = np.asarray(strata, dtype=np.int64)
    T, G = traits.shape[0], genes.shape[0]
    lab, val = (traits == 1), (traits != 2)
    a, m = np.zeros((T, G, S), dtype=np.int64), np.zeros((T, G, S), dtype=np.int64)
    for g in range(G):
        idx = np.flatnonzero(genes[g])
        st = strata[idx]
        for t in range(T):
            a[t, g] = np.bincount(st[lab[t, idx]], minlength=S)
            m[t, g] = np.bincount(st[val[t, idx]], minlength=S)
    k = np.stack([np.bincount(strata[lab[t]], minlength=S) for t in range(T)])
    n = np.stack([np.bincount(strata[val[t]], minlength=S) for t in range(T)])
    return a, m, k, n


def tables(a, m, k, n, t, g):
    """The (a, m, k, n) of every stratum of one (trait, gene), as cmh_spec takes them."""
    return list(zip(a[t, g].tolist(), m[t, g].tolist(), k[t].tolist(), n[t].tolist()))


def restate(a, m, k, n):
    """cmh_spec.cmh of every (trait, gene): dict of float64 [T, G] (stat, p, odds, e2, var), a int64 [T, G] and crit
    uint32 [T, G, 2]."""
    T, G, _S = a.shape
    want = {key: np.empty((T, G)) for key in ("stat", "p", "odds", "e2", "var")}
    want["a"] = np.empty((T, G), dtype=np.int64)
    want["crit"] = np.empty((T, G, 2), dtype=np.uint32)
    for t in range(T):
        kt, nt = k[t].tolist(), n[t].tolist()
        for g in range(G):
            r = S10.cmh(list(zip(a[t, g].tolist(), m[t, g].tolist(), kt, nt)))
            for key in want:
                want[key][t, g] = r[key]
    return want


def check_p(got, want, tiny=0.0):
    """|dp| <= 1e-12 and <= 1e-10 |p| against math.erfc (erfc amplifies the few ulp of the device
    erfc by about 2 x^2, which is the statistic itself: below 1e4 on every shape tested, so a few ulp become some
    1e-12 relative at the most; test_gpu_cmh_limits.py asserts that margin).  ``tiny``: wanted values below it
    (subnormals and 0 with tiny = P_NORMAL) are held to the absolute bound and to got >= 0 only.  Returns
    (max abs error, max relative error, index of the latter)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    rel = np.where(want >= tiny, err / np.where(want > 0, want, 1.0), 0.0)
    worst = np.unravel_index(int(np.argmax(rel)), rel.shape)
    print("cmh p: max abs error %.3e, max relative error %.3e" % (err.max(), rel.max()))
    assert (got >= 0).all()
    assert err.max() <= 1e-12 and rel.max() <= 1e-10
    return float(err.max()), float(rel.max()), worst


def random_genes_traits(G, N, T, S, dense_genes=False):
    """Random genes with carrier frequencies across [0.02, 0.98] (or [0.3, 0.7]), gene 1 in no and gene 2 in every
    isolate, gene 3 strongly associated with trait 0; missing values in the last trait."""
    rng = np.random.default_rng(G + N + S)
    lo, hi = (0.3, 0.7) if dense_genes else (0.02, 0.98)
    genes = (rng.random((G, N)) < rng.uniform(lo, hi, (G, 1))).astype(np.uint8)
    genes[1], genes[2] = 0, 1
    traits = (rng.random((T, N)) < rng.uniform(0.2, 0.8, (T, 1))).astype(np.uint8)
    traits[0] = np.where(rng.random(N) < 0.7, genes[3], traits[0])              # one strong association
    traits[T - 1, rng.random(N) < 0.06] = 2
    return genes, traits, rng


# -- A: the largest shape the library takes ---------------------------------------------------------------------
LIMIT_N, LIMIT_S, LIMIT_T = 20479, 1024, 5
LIMIT_GENES = {"interleaved": 40, "blocked": 40, "two_level": 300}


def limit_strata(name):
    """The strata of a limit layout, int64 [LIMIT_N] with indices in [0, LIMIT_S)."""
    N, S = LIMIT_N, LIMIT_S
    i = np.arange(N)
    if name == "interleaved":            # members of a stratum 1024 isolates = 32 words apart: one segment per isolate
        return i % S
    rng = np.random.default_rng(1024)
    if name == "blocked":
        sizes = rng.integers(2, 34, S)
        sizes[rng.choice(S, 60, replace=False)] = 1
        sizes[rng.choice(S, 30, replace=False)] = rng.integers(33, 65, 30)      # more than one word of members
        sizes[rng.choice(S, 30, replace=False)] = rng.integers(65, 140, 30)     # more than two
        sizes[[0, 511, 512, 513, S - 1]] = 0                                    # indices without any member
        big = int(np.argmax(sizes))
        sizes[big] += N - sizes.sum()                                           # the largest block takes the remainder
        assert sizes[big] > 64 and sizes.sum() == N
        return np.repeat(np.arange(S), sizes)
    assert name == "two_level"
    # blocks of 150 .. 700 isolates; inside a block two (every third block: three) strata take the isolates in turn
    strata, s, at, b = np.empty(N, dtype=np.int64), 3, 0, 0
    while at < N:
        size = min(int(rng.integers(150, 700)), N - at)
        ways = 3 if b % 3 == 2 else 2
        ids = np.array([s + 7 * w for w in range(ways)])                        # indices apart, not ascending in step
        strata[at:at + size] = ids[np.arange(size) % ways]
        s, at, b = s + 7 * ways + 1, at + size, b + 1
    assert strata.max() < S - 1
    strata[strata == strata.max()] = S - 1                                      # the last index has members
    return strata


def limit_case(name):
    """(genes uint8 [G, N], traits uint8 [5, N], strata) of a limit layout."""
    N, T, G = LIMIT_N, LIMIT_T, LIMIT_GENES[name]
    strata = limit_strata(name)
    genes, traits, rng = random_genes_traits(G, N, T, {"interleaved": 1, "blocked": 2, "two_level": 3}[name])
    traits[2, rng.random(N) < 0.3] = 2                                          # missing values in traits 2 and 4
    if name == "blocked":
        traits[1, strata == 7] = 2                                              # a stratum emptied for one trait
    return genes, traits, strata


# -- B: the region's clamps and ties, on purpose ----------------------------------------------------------------
EDGE_NK = ((8, 4), (8, 4), (12, 6), (1, 1), (1, 0), (30, 3), (40, 30), (2, 1), (64, 32), (33, 5))   # (n, k) per stratum
# genes as (a, m) per stratum; what each is there for (asserted in test_cmh_spec.py)
EDGE_GENES = {
    "dead": ((4, 8), (0, 0), (0, 0), (0, 0), (0, 1), (3, 30), (0, 0), (1, 2), (0, 0), (5, 33)),
    "a_equals_e": ((4, 8), (0, 4), (4, 4), (0, 0), (0, 1), (0, 0), (0, 0), (1, 2), (32, 64), (0, 0)),
    "inside_cc": ((0, 0), (0, 1), (6, 12), (1, 1), (0, 1), (3, 30), (0, 0), (1, 2), (0, 0), (0, 0)),
    "lo_clamp": ((0, 0), (0, 0), (0, 0), (1, 1), (0, 1), (2, 7), (0, 0), (0, 0), (0, 0), (5, 6)),
    "hi_clamp": ((4, 8), (2, 6), (1, 7), (0, 0), (0, 1), (1, 16), (30, 40), (1, 2), (3, 35), (0, 28)),
    "mirror_tie": ((0, 2), (4, 8), (0, 0), (1, 1), (0, 0), (0, 0), (0, 0), (1, 2), (0, 0), (5, 33)),
    "odds_inf": ((0, 0), (4, 8), (2, 2), (1, 1), (0, 0), (3, 30), (14, 14), (0, 0), (0, 0), (5, 33)),
    "none": tuple((0, 0) for _ in EDGE_NK),
    "all": tuple((k, n) for n, k in EDGE_NK),
}


def edge_case():
    """(genes [G, N], traits [2, N], strata [N], names): the genes of EDGE_GENES expanded to isolates -- a stratum's
    k positives first, the gene in the first a of them and in the first m - a of the negatives -- plus a few random
    genes.  Trait 0 has no missing value; trait 1 is trait 0 with stratum 7 (n = 2) and stratum 3 (n = 1) masked
    away altogether (n = 0) and all but one isolate of stratum 0 masked (n = 1)."""
    names = list(EDGE_GENES)
    trait, strata, cols = [], [], {name: [] for name in names}
    for s, (n, k) in enumerate(EDGE_NK):
        trait += [1] * k + [0] * (n - k)
        strata += [s] * n
        for name in names:
            a, m = EDGE_GENES[name][s]
            assert max(0, k + m - n) <= a <= min(k, m)
            cols[name] += [1] * a + [0] * (k - a) + [1] * (m - a) + [0] * (n - k - (m - a))
    genes = np.array([cols[name] for name in names], dtype=np.uint8)
    N = genes.shape[1]
    rng = np.random.default_rng(10)
    genes = np.concatenate([genes, (rng.random((7, N)) < rng.uniform(0.1, 0.9, (7, 1))).astype(np.uint8)])
    strata = np.array(strata)
    masked = np.array(trait, dtype=np.uint8)
    masked[(strata == 7) | (strata == 3)] = 2
    masked[np.flatnonzero(strata == 0)[1:]] = 2
    return genes, np.stack([np.array(trait, dtype=np.uint8), masked]), strata, names


# -- C: p at large statistics -----------------------------------------------------------------------------------
def graded_case():
    """(genes [G, N], traits [1, N], strata) with N = 6000 and four strata of unequal sizes: the genes are copies of
    the trait with a fixed number of isolates flipped -- agreement from 55 % to 100 %, graded finely where the
    statistic passes 1400 .. 1500 and p leaves the normal doubles."""
    N = 6000
    rng = np.random.default_rng(6000)
    strata = np.searchsorted(np.array([700, 2500, 2600]), np.arange(N), side="right")
    strata = strata[rng.permutation(N)]
    trait = (rng.random(N) < 0.45).astype(np.uint8)
    agree = np.concatenate([np.linspace(0.55, 1.0, 91), np.linspace(0.735, 0.765, 121)])
    genes = np.empty((len(agree), N), dtype=np.uint8)
    for g, f in enumerate(agree):
        flip = rng.permutation(N)[:N - int(round(f * N))]
        genes[g] = trait
        genes[g, flip] ^= 1
    return genes, trait[None], strata


# -- D: associate(cmh=True) over several label batches ----------------------------------------------------------
#        name             G    N      T  S  P     perms per batch, tile dwords (None: the dense kernels)
BATCH_CASES = {
    "lists_tw8": (130, 2600, 2, 5, 1100, 512, 8),
    "lists_tw4": (70, 5200, 1, 9, 700, 512, 4),
    "lists_tw2": (40, 10_300, 1, 3, 600, 512, 2),
    "dense": (130, 2600, 2, 5, 500, 200, None),
}


def batch_case(name):
    """(genes, traits, strata, S, P, batch, tile dwords) of a D case: random strata, gene frequencies across
    [0.02, 0.98] so that some genes are carried by more than half of the isolates."""
    G, N, T, S, P, batch, tw = BATCH_CASES[name]
    genes, traits, rng = random_genes_traits(G, N, T, S)
    assert (genes.sum(1) > N // 2).any() and (genes.sum(1) < N // 2).any()
    return genes, traits, rng.integers(0, S, N), S, P, batch, tw


def exact_rule_mismatches(tabs, crit, counts):
    """The counts among ``counts`` at which the region ``crit`` and the exact rule (Fractions) part by more than
    S10 allows: a count in the region that is not exactly extreme must have its distance within tau + 2e-8 of the
    observed one, and every exactly extreme count must be in the region."""
    A, E, _V = S10.exact(tabs)
    slack = Fraction(S10.TAU) + Fraction(2, 10 ** 8)
    bad = []
    for ap in counts:
        ap = int(ap)
        got, ex = bool(S10.in_region(crit, ap)), bool(S10.exact_extreme(tabs, ap))
        if got != ex and (ex or abs(abs(ap - E) - abs(A - E)) > slack):
            bad.append(ap)
    return bad


def subsample_pairs(T, G, count=20):
    """About ``count`` (trait, gene) pairs spread evenly over [T, G]."""
    flat = np.unique(np.linspace(0, T * G - 1, count).astype(np.int64))
    return [(int(f) // G, int(f) % G) for f in flat]


# -- what the device tests of S10, S12, S13 and S14 hold a result to: the fixed-shape files and the randomised corpus
#    (strata_stress_cases.py) call the same functions, so both stand at the same bounds ------------------------------
def check_cmh(out, want):
    """cmh()'s result as numpy arrays against ``restate``'s of the same pairs: stat, e2, var and odds bit for bit,
    the region, nan and p = 1 exactly where no stratum is informative, p within check_p."""
    for key in ("stat", "e2", "var", "odds"):
        assert np.array_equal(out[key], want[key], equal_nan=True), key
    assert np.array_equal(out["crit"].view(np.uint32), want["crit"])
    dead = want["var"] == 0
    assert np.array_equal(np.isnan(out["stat"]), dead) and (out["p"][dead] == 1.0).all()
    check_p(out["p"], want["p"])
    return dead


def check_exact_pairs(c, got, pairs, what, reference=S12.reference, allow_ties=0):
    """The pairs ``pairs`` of a case against the reference: table, p (bit-identical to its table entry), p_region.
    Near-tied pairs are dropped from the p comparison (at most ``allow_ties`` of them); returns how many were."""
    a, m, k, n = c.recount()
    tab_got, tab_want, p_got, p_want, r_got, r_want, ties = [], [], [], [], [], [], 0
    for t, g in pairs:
        tabs = tables(a, m, k, n, t, g)
        ref = reference(tabs)
        lo, tab, p, region = ref[:4]
        o = got["off"][t * c.G + g]
        row = got["tab"][o:got["off"][t * c.G + g + 1]]
        assert got["lo"][t, g] == lo and len(row) == len(tab), (t, g)
        assert got["a"][t, g] == S10.cmh(tabs)["a"] and tuple(got["crit"][t, g]) == tuple(S10.cmh(tabs)["crit"])
        assert got["p"][t, g] == row[got["a"][t, g] - lo], (t, g)          # the gene's own entry, bit for bit
        assert row.max() == 1.0 and row.min() >= 0.0
        if len(ref) > 4 and ref[4]:
            ties += 1
            continue
        tab_got.append(row), tab_want.append(tab), p_got.append(got["p"][t, g]), p_want.append(p)
        r_got.append(got["p_region"][t, g]), r_want.append(region)
    assert ties <= allow_ties, "%d near-tied pairs" % ties
    if tab_got:
        S12.check(np.concatenate(tab_got), np.concatenate(tab_want), what + ", tables")
        S12.check(p_got, p_want, what + ", p")
        S12.check(r_got, r_want, what + ", p_region")
    return ties


ODDS_EPS = 1e-12
ODDS_EXACT_BUDGET = 1_000_000     # sum of L^2 over the pairs of a case that take the exact check (about a second)


def check_odds_case(c, got, a_dev, level, what, pairs=None):
    """cmh_exact_odds() as float64 [3, T, G] (odds, lower, upper): every pair of ``pairs`` (default: all) against the
    references; returns {"special": counts of the exact values met, "L": the support sizes, "unspecified": pairs with
    f(A) < 1e-290}."""
    half = S13.half_of(level)
    a, m, k, n = c.recount()
    pairs = [(t, g) for t in range(c.T) for g in range(c.G)] if pairs is None else pairs
    sampled = set(subsample_pairs(c.T, c.G, 200)) & set(pairs) if len(pairs) > 200 else set(pairs)
    budget, exact, worst, seen = ODDS_EXACT_BUDGET, 0, 0.0, {"zero": 0, "inf": 0, "nan": 0, "L": [], "unspecified": 0}
    for t, g in pairs:
        tabs = tables(a, m, k, n, t, g)
        lo, f = S12.float_pmf(tabs)
        A, L = S10.cmh(tabs)["a"], len(f)
        assert a_dev[t, g] == A
        seen["L"].append(L)
        mine = tuple(float(v) for v in got[:, t, g])
        if L > 1 and f[A - lo] < S12.TINY:
            seen["unspecified"] += 1
            assert all(v >= 0 for v in mine), (what, t, g, mine)                # (nan >= 0 is False)
            continue
        if (t, g) in sampled and 1 < L <= 600 and budget >= L * L:
            budget -= L * L
            exact += 1
            weights = S12.exact_weights(tabs)
            for which, v in zip(S13.WHICH, mine):
                want = S13.special(tabs, which)
                if want is None:
                    assert math.isfinite(v) and v > 0 and S13.brackets(tabs, half, v, which, ODDS_EPS, weights), \
                        (what, t, g, which, v, S13.restate_pmf(f, A - lo, half))
                else:
                    assert v == want, (what, t, g, which, v, want)
        else:
            worst = max(worst, S13.check_values(mine, S13.restate_pmf(f, A - lo, half), (what, t, g)))
        seen["zero"] += mine[0] == 0.0
        seen["inf"] += mine[0] == math.inf
        seen["nan"] += math.isnan(mine[0])
        if L > 1:
            assert mine[1] <= mine[0] <= mine[2], (what, t, g, mine)
    print("cmh exact odds %s, level %s: %d pairs, %d by the exact check at 1e-12, the others within %.2e relative of "
          "the restatement; supports of %d to %d entries; %d at 0, %d at inf, %d nan, %d unspecified"
          % (what, level, len(pairs), exact, worst, min(seen["L"]), max(seen["L"]), seen["zero"], seen["inf"],
             seen["nan"], seen["unspecified"]))
    return seen, exact


HOMOG_P_SPECIFIED = 1e-290           # S14: below it any p in [0, 1e-290] stands for the true one


def check_homog_case(c, got, odds, what, pairs=None):
    """cmh_homogeneity() as numpy arrays and the odds ratios of cmh() it read: the pairs of ``pairs`` (default: all)
    against the restatement; returns (defined rows, undefined rows, the largest df)."""
    a, m, k, n = c.recount()
    pairs = [(t, g) for t in range(c.T) for g in range(c.G)] if pairs is None else pairs
    defined = undefined = 0
    worst_p, top_df = 0.0, 0
    for t, g in pairs:
        tabs = tables(a, m, k, n, t, g)
        psi = float(odds[t, g])
        want = S10.cmh(tabs)["odds"]
        assert psi == want or (math.isnan(psi) and math.isnan(want)), (what, t, g, psi, want)
        bd, tarone, df, _p = S14.homogeneity(tabs, psi)
        mine = (float(got["stat_bd"][t, g]), float(got["stat_tarone"][t, g]), int(got["df"][t, g]),
                float(got["p"][t, g]))
        if df == 0:
            undefined += 1
            assert math.isnan(mine[0]) and math.isnan(mine[1]) and mine[2:] == (0, 1.0), (what, t, g, mine)
            continue
        defined += 1
        top_df = max(top_df, df)
        assert mine[:3] == (bd, tarone, df), (what, t, g, psi, mine, (bd, tarone, df))     # the restatement's bits
        p_want = S14.chi2_sf(mine[1], mine[2])
        assert 0.0 <= mine[3] <= 1.0
        if p_want >= HOMOG_P_SPECIFIED:
            err = abs(mine[3] - p_want) / p_want
            worst_p = max(worst_p, err)
            assert err <= 1e-10, (what, t, g, mine, p_want)
        else:
            assert mine[3] <= HOMOG_P_SPECIFIED, (what, t, g, mine, p_want)
        if mine[1] == 0.0:
            assert mine[3] == 1.0
    print("cmh homogeneity %s: %d pairs, %d defined (bit for bit), %d undefined, df up to %d, p within %.2e relative"
          % (what, len(pairs), defined, undefined, top_df, worst_p))
    return defined, undefined, top_df
