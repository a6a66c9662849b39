"""The restatement of spec S22 (cat_wy_spec.py) against the rationals and against S20's and S21's own counts: the
statistic is X2 to rounding, the band below the observed statistic catches every exact exceedance, the family-wise
count dominates the per-gene count and meets it for a single gene, and the maxima compose over batches."""
from fractions import Fraction

import numpy as np

import cat_wy_spec as ws
import categorical_spec as cs
import gcmh_spec as gs

SEED = 0x5EEDCA7E22
TIE_TRAITS = ([3, 3, 3], [6, 3, 12])                    # class sizes whose permuted tables tie exactly (S20)


def _problem(rng, k):
    """One small trait: (genes [G][N], codes [N], K, strata [N], S).  Every third is a tie trait, the others have K =
    2 .. 8 classes; missing labels and an empty class come and go."""
    if k % 3 == 0:
        codes = np.repeat(np.arange(1, 4), TIE_TRAITS[(k // 3) % 2])
        K = 3
    else:
        K = 2 + k % 7
        N = int(rng.integers(max(4, K), 26))
        codes = rng.integers(1, K + 1, N)
        if k % 4 == 1 and K > 2:
            codes[codes == 2] = 1                       # an empty class in the middle
        if k % 5 == 2:
            codes[codes == K] = 1                       # the last class is empty
    codes = codes.copy()
    rng.shuffle(codes)
    if k % 2:
        codes[rng.random(len(codes)) < 0.2] = 0         # isolates without a label
    N = len(codes)
    G = 1 + k % 5
    genes = (rng.random((G, N)) < rng.uniform(0.1, 0.9, (G, 1))).astype(int)
    if G > 2:
        genes[1] = 0                                    # untestable: m = 0
        genes[2] = 1                                    # untestable: m = n
    S = 1 + k % 3
    strata = rng.integers(0, S, N)
    strata[0] = S - 1
    return genes.tolist(), codes.tolist(), K, strata.tolist(), S


def test_s_is_the_chi_square_to_rounding():
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in range(200):
        genes, codes, K, _st, _S = _problem(rng, k)
        pr = ws.chi2_problem(genes, codes, K)
        for a, ivm, s in zip(pr["a"], pr["ivm"], pr["s_obs"]):
            if not cs.testable(a, pr["nk"]):
                assert (ivm, s) == (0.0, 0.0)
                continue
            exact = cs.x2_exact(a, pr["nk"])
            err = abs(Fraction(s) - exact)
            assert err <= Fraction(1, 10 ** 14) * exact
            worst = max(worst, float(err / exact) if exact else 0.0)
            assert abs(s - cs.statistic(a, pr["nk"])[1]) <= 1e-14 * s          # S20's x2, close but not the same bits
    print("worst relative error of s against the rational X2: %.3g" % worst)
    # at the largest table the terms stay exact integers before they are rounded once
    n = cs.MAX_ISOLATES
    nk = [n // 2, n - n // 2]
    a = [n // 2, 0]
    s = ws.stat(a, nk, ws.ivm_of(a, nk))
    assert abs(Fraction(s) - cs.x2_exact(a, nk)) <= Fraction(1, 10 ** 14) * n and abs(s - n) <= 1e-10


def test_the_band_catches_every_exact_exceedance():
    """Exact X2_pi >= X2_obs implies s_pi >= thr -- ties between distinct tables included."""
    rng = np.random.default_rng(2)
    exceed = ties = 0
    for k in range(200):
        genes, codes, K, _st, _S = _problem(rng, k)
        pr = ws.chi2_problem(genes, codes, K)
        rows = [cs.perm_row(SEED, k, pi, codes) for pi in range(30)]
        for g, gene in enumerate(genes):
            for row in rows:
                a = cs.table(gene, row, K)
                if cs.exceeds(a, pr["a"][g], pr["nk"]):
                    exceed += 1
                    ties += a != pr["a"][g] and cs.s_exact(a, pr["nk"]) == cs.s_exact(pr["a"][g], pr["nk"])
                    assert ws.stat(a, pr["nk"], pr["ivm"][g]) >= pr["thr"][g], (k, g, a)
    assert exceed > 5000 and ties > 50                  # the property was put to the test, exact ties among them


def test_r_fwer_dominates_r_and_meets_it_for_one_gene():
    rng = np.random.default_rng(3)
    P = 24
    singles = in_band = 0
    for k in range(200):
        genes, codes, K, strata, S = _problem(rng, k)
        G = len(genes)
        # chi-square
        pr = ws.chi2_problem(genes, codes, K)
        rows = [cs.perm_row(SEED, k, pi, codes) for pi in range(P)]
        mx = ws.maxs(ws.chi2_cells(genes, rows, pr, K))
        rf = ws.r_fwer(mx, pr["thr"])
        r = [cs.r_count(g, rows, codes, K) for g in genes]
        assert (rf >= np.array(r)).all(), k
        for g in range(G):
            if not cs.testable(pr["a"][g], pr["nk"]) or pr["s_obs"][g] == 0.0:
                assert rf[g] == P == r[g]
        order = np.argsort(pr["s_obs"], kind="stable")
        assert (np.diff(rf[order]) <= 0).all()          # r_fwer does not increase with s_obs
        if G == 1:
            band = any(ws.inside_band(cs.table(genes[0], row, K), pr["a"][0], pr["nk"]) for row in rows)
            in_band += band
            if not band:
                singles += 1
                assert rf[0] == r[0], k
        # generalized CMH
        pq = ws.gcmh_problem(genes, codes, strata, S)
        qrows = [gs.perm_row(SEED, k, pi, codes, strata, S) for pi in range(P)]
        cells = ws.gcmh_cells(genes, qrows, pq, strata, S)
        mq = ws.maxs(cells)
        rq = ws.r_fwer(mq, pq["thr"])
        r_own = (cells >= np.array(pq["thr"])[None, :]).sum(axis=0)
        assert (rq >= r_own).all(), k
        for g in range(G):
            if pq["st"][g]["df"] == 0:
                assert pq["s_obs"][g] == 0.0 and rq[g] == P == r_own[g]
        order = np.argsort(pq["thr"], kind="stable")
        assert (np.diff(rq[order]) <= 0).all()
        if G == 1:
            assert rq[0] == r_own[0], k
    assert singles >= 30 and in_band == 0


def test_maxs_composes_over_batches():
    rng = np.random.default_rng(4)
    genes, codes, K, strata, S = _problem(rng, 4)
    pr = ws.chi2_problem(genes, codes, K)
    rows = [cs.perm_row(SEED, 0, pi, codes) for pi in range(20)]
    whole = ws.maxs(ws.chi2_cells(genes, rows, pr, K))
    parts = np.concatenate([ws.maxs(ws.chi2_cells(genes, rows[:7], pr, K)),
                            ws.maxs(ws.chi2_cells(genes, rows[7:], pr, K))])
    assert np.array_equal(whole, parts)
    pq = ws.gcmh_problem(genes, codes, strata, S)
    qrows = [gs.perm_row(SEED, 0, pi, codes, strata, S) for pi in range(20)]
    whole = ws.maxs(ws.gcmh_cells(genes, qrows, pq, strata, S))
    parts = np.concatenate([ws.maxs(ws.gcmh_cells(genes, qrows[:7], pq, strata, S)),
                            ws.maxs(ws.gcmh_cells(genes, qrows[7:], pq, strata, S))])
    assert np.array_equal(whole, parts)


def test_the_array_route_is_the_scalar_one():
    rng = np.random.default_rng(5)
    for k in range(40):
        genes, codes, K, _st, _S = _problem(rng, k)
        pr = ws.chi2_problem(genes, codes, K)
        rows = [cs.perm_row(SEED, k, pi, codes) for pi in range(5)]
        a = np.array([[cs.table(g, row, K) for g in genes] for row in rows])
        assert np.array_equal(ws.stats(a, pr["nk"], pr["ivm"]), ws.chi2_cells(genes, rows, pr, K))
        assert np.array_equal(ws.stats(pr["a"], pr["nk"], pr["ivm"]), np.array(pr["s_obs"]))
    assert ws.ONE_MINUS_BAND == 1.0 - 1e-9 and ws.thr_of(2.0) == 2.0 * (1.0 - 1e-9)
