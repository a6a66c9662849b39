"""Spec S24's restatement (score_spec.py) held to anchors that share no code with it: Pearson's X2 of the 2 x 2 table
for the logistic score statistic without covariates, numpy's least squares on the full model for the linear
coefficient and its t, the finite sums of Student's distribution and SciPy for the tail, the score equations and
scikit-learn for the logistic null fit; every untestable and every skipped-trait branch; and the engine's numpy host
side against the restatement.  CPU only."""
import math

import mpmath
import numpy as np
import pytest

import categorical_spec as cs
import score_spec as ss

SIZES = (33, 64, 65, 200, 513)
REL = 1e-10                   # the project's bar for a value that passes a solver (S14, S15)
MAX_REDRAWN = 0.05


def _rel(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


def _draw(rng, N, c, kind):
    """One trait of the issue's law: standard-normal covariates, log odds (or a mean) of unit scale, some cells
    missing."""
    cov = rng.standard_normal((c, N))
    eta = (cov.T @ rng.standard_normal(c) / math.sqrt(c) if c else np.zeros(N)) + 0.3 * rng.standard_normal()
    if kind == "logistic":
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        y = eta + rng.standard_normal(N)
    if N > 40:
        y[rng.random(N) < 0.05] = np.nan
        if c:
            cov[rng.integers(c), rng.integers(N)] = np.nan
    return y, cov


def _problems(kind, count, seed):
    """``count`` fitted traits (N cycling through SIZES, c uniform in 0 .. 8); a trait whose null fit S24 refuses is
    redrawn, and at most 5 % of the draws may be."""
    rng = np.random.default_rng(seed)
    out, draws, redrawn = [], 0, 0
    while len(out) < count:
        N = SIZES[len(out) % len(SIZES)]
        c = int(rng.integers(0, 9))
        y, cov = _draw(rng, N, c, kind)
        draws += 1
        try:
            fit = ss.null_fit(list(y), [list(col) for col in cov], kind)
        except ss.Refused:
            redrawn += 1
            continue
        out.append((N, c, y, cov, fit))
    assert redrawn <= MAX_REDRAWN * draws, "%d of %d draws were refused" % (redrawn, draws)
    return out


@pytest.fixture(scope="module")
def logistic_problems():
    return _problems("logistic", 40, 2401)


@pytest.fixture(scope="module")
def linear_problems():
    return _problems("linear", 40, 2402)


def _genes(rng, N, count):
    return (rng.random((count, N)) < rng.uniform(0.1, 0.9, (count, 1))).astype(np.uint8)


def test_logistic_without_covariates_is_pearsons_chi_square():
    """c = 0: the score statistic is the uncorrected Pearson X2 of the 2 x 2 table, by categorical_spec at K = 2 and
    by scipy.stats.chi2_contingency(correction=False), within 1e-10 relative; and the tails agree."""
    from scipy.stats import chi2_contingency
    rng = np.random.default_rng(11)
    seen = 0
    for N in SIZES:
        for _ in range(4):
            y = (rng.random(N) < rng.uniform(0.2, 0.8)).astype(np.float64)
            y[rng.random(N) < 0.1] = np.nan
            fit = ss.null_fit(list(y), [], "logistic")
            rows, valid, packed = ss.plan_rows(fit, N)
            codes = [0 if math.isnan(v) else int(v) + 1 for v in y]
            nk = cs.sizes(codes, 2)
            for gene in _genes(rng, N, 6):
                got = ss.statistic(list(gene), rows, valid, packed, "logistic")
                a = cs.table(list(gene), codes, 2)
                ok, x2, _df, p, _v = cs.statistic(a, nk)
                assert got["testable"] == ok
                if not ok:
                    continue
                table = [[a[0], a[1]], [nk[0] - a[0], nk[1] - a[1]]]
                assert _rel(got["stat"], x2) <= REL
                assert _rel(got["stat"], chi2_contingency(table, correction=False)[0]) <= REL
                assert _rel(ss.p_of("logistic", got["stat"], got["df"]), p) <= REL
                seen += 1
    assert seen >= 100


def test_linear_is_least_squares_on_the_full_model(linear_problems):
    """beta and t^2 of the score quantities against numpy.linalg.lstsq with the gene as a column of the full model,
    within 1e-10 relative."""
    rng = np.random.default_rng(12)
    seen = 0
    for N, c, y, cov, fit in linear_problems:
        rows, valid, packed = ss.plan_rows(fit, N)
        V = fit["V"]
        X = np.array(fit["X"])
        for gene in _genes(rng, N, 4):
            got = ss.statistic(list(gene), rows, valid, packed, "linear", fit["rss"])
            if not got["testable"]:
                continue
            full = np.column_stack([X, gene[V].astype(np.float64)])
            coef, _res, rank, _sv = np.linalg.lstsq(full, y[V], rcond=None)
            assert rank == full.shape[1]
            resid = y[V] - full @ coef
            df = len(V) - full.shape[1]
            assert df == got["df"]
            cov_gene = np.linalg.inv(full.T @ full)[-1, -1]
            t2 = coef[-1] ** 2 / (float(resid @ resid) / df * cov_gene)
            assert _rel(got["beta"], coef[-1]) <= REL, (N, c)
            assert _rel(got["stat"] ** 2, t2) <= REL, (N, c)
            seen += 1
    assert seen >= 120


def _t_tail_by_finite_sum(t, df):
    """P(|T_df| >= |t|) = 1 - A(t | df) by the finite trigonometric sums of Abramowitz & Stegun 26.7.3 / 26.7.4, at
    400 digits (the sum cancels down to the tail)."""
    with mpmath.workdps(400):
        theta = mpmath.atan(abs(mpmath.mpf(t)) / mpmath.sqrt(df))
        s, c = mpmath.sin(theta), mpmath.cos(theta)
        if df % 2:
            total, term = mpmath.mpf(0), c
            for k in range(1, df - 1, 2):                   # cos + 2/3 cos^3 + (2 4)/(3 5) cos^5 + ... + cos^(df - 2)
                total += term
                term = term * c * c * (k + 1) / (k + 2)
            return 1 - 2 / mpmath.pi * (theta + s * total)
        total, term = mpmath.mpf(0), mpmath.mpf(1)
        for k in range(0, df - 1, 2):                       # 1 + 1/2 cos^2 + (1 3)/(2 4) cos^4 + ... + cos^(df - 2)
            total += term
            term = term * c * c * (k + 1) / (k + 2)
        return 1 - s * total


def test_the_t_tail_of_the_restatement():
    """The restatement's tail (mpmath's incomplete beta function at 50 digits) against the finite sums of the t
    distribution for an integer df, and SciPy's 2 t.sf, which is itself some 2e-13 off at t = 38, df = 1990: 1e-10
    relative."""
    from scipy.stats import t as student
    for t, df in ((0.0, 5), (1e-6, 3), (0.3, 1), (1.0, 2), (2.5, 7), (5.0, 30), (15.0, 2000), (38.0, 1990), (-4.0, 11),
                  (60.0, 40), (1.7, 511), (9.0, 23), (2.0, 4), (3.0, 3)):
        got = ss.t_sf2(t, df)
        want = _t_tail_by_finite_sum(t, df)
        assert abs(got - want) <= mpmath.mpf(REL) * want, (t, df)
        assert _rel(float(got), 2.0 * student.sf(abs(t), df)) <= REL, (t, df)
    assert ss.t_sf2(math.inf, 4) == 0 and ss.p_of("linear", 0.0, 4) == 1.0


def test_linear_p_is_the_tail_at_the_statistic(linear_problems):
    rng = np.random.default_rng(13)
    from scipy.stats import t as student
    for N, c, y, cov, fit in linear_problems[:10]:
        rows, valid, packed = ss.plan_rows(fit, N)
        for gene in _genes(rng, N, 2):
            got = ss.statistic(list(gene), rows, valid, packed, "linear", fit["rss"])
            if got["testable"]:
                p = float(ss.p_of("linear", got["stat"], got["df"]))
                assert _rel(p, 2.0 * student.sf(abs(got["stat"]), got["df"])) <= REL


def test_the_logistic_null_fit_solves_the_score_equations(logistic_problems):
    """max_j |sum x_ij (y_i - mu_i)| <= q n / 4 1e-10: the step bound times the largest possible norm of A."""
    for N, c, y, cov, fit in logistic_problems:
        q, n = fit["q"], fit["n"]
        worst = max(abs(sum(xi[j] * ri for xi, ri in zip(fit["X"], fit["r"]))) for j in range(q))
        assert worst <= q * n / 4.0 * 1e-10, (N, c, worst)
        assert all(abs(x) <= 1.0 for xi in fit["X"] for x in xi)


# what scikit-learn's newton-cholesky solver at tol 1e-12 reached against the restatement over the problems below:
# the largest |coefficient difference| was 1.53e-11; the bar is a decade above it
SKLEARN_BAR = 1.6e-10


def test_the_logistic_null_fit_agrees_with_scikit_learn(logistic_problems):
    """The converged coefficients against sklearn.linear_model.LogisticRegression(penalty=None) on the same scaled
    columns, to the accuracy that solver reaches: its newton-cholesky solver at tol 1e-12 was measured 1.53e-11 off
    the restatement (largest absolute coefficient difference over these problems; a looser solver of the same class
    was measured 1.7e-9 off when the feature was specified); the bar is 1.6e-10, a decade above the measurement."""
    from sklearn.linear_model import LogisticRegression
    worst = 0.0
    for N, c, y, cov, fit in logistic_problems:
        if c == 0:
            continue
        X = np.array(fit["X"])[:, 1:]
        model = LogisticRegression(penalty=None, solver="newton-cholesky", tol=1e-12, max_iter=1000)
        model.fit(X, y[fit["V"]].astype(int))
        got = np.concatenate([model.intercept_, model.coef_[0]])
        worst = max(worst, float(np.max(np.abs(got - np.array(fit["beta"])))))
    print("largest |coefficient difference| against scikit-learn: %.3g" % worst)
    assert worst <= SKLEARN_BAR


def test_every_untestable_branch():
    rng = np.random.default_rng(14)
    N = 65
    cov = rng.standard_normal((2, N))
    cov[1] = (rng.random(N) < 0.4).astype(np.float64)              # a 0 / 1 covariate
    y = (rng.random(N) < 0.5).astype(np.float64)
    y[:5] = np.nan
    for kind in ("logistic", "linear"):
        fit = ss.null_fit(list(y), [list(col) for col in cov], kind)
        rows, valid, packed = ss.plan_rows(fit, N)
        every = [1] * N
        only_invalid = [1] * 5 + [0] * (N - 5)
        like_covariate = [int(v) for v in cov[1]]
        for gene, what in (([0] * N, "m = 0"), (every, "m = n"), (only_invalid, "m = 0 among the valid"),
                           (like_covariate, "Vg cut")):
            got = ss.statistic(gene, rows, valid, packed, kind, fit["rss"])
            assert not got["testable"] and got["stat"] == 0.0 and got["beta"] == 0.0 and got["se"] == 0.0, what
            assert ss.p_of(kind, got["stat"], got["df"], got["testable"]) == 1.0
        got = ss.statistic(like_covariate, rows, valid, packed, kind, fit["rss"])
        assert 0 < got["m"] < fit["n"] and got["Vg"] <= ss.VG_CUT * got["b"][0]
        one = [0] * N
        one[7] = 1
        assert ss.statistic(one, rows, valid, packed, kind, fit["rss"])["testable"]
    # the linear kind's own: a gene that leaves no residual has an infinite t and p 0
    z = rng.standard_normal(N)
    gene = [int(v) for v in (rng.random(N) < 0.5)]
    fit = ss.null_fit([float(g) for g in gene], [list(z)], "linear")
    rows, valid, packed = ss.plan_rows(fit, N)
    got = ss.statistic(gene, rows, valid, packed, "linear", 0.0)   # rss below what the gene explains
    assert got["testable"] and got["stat"] == math.inf and got["se"] == 0.0
    assert ss.p_of("linear", got["stat"], got["df"]) == 0


def test_every_skipped_trait_branch():
    rng = np.random.default_rng(15)
    N = 40
    y = (rng.random(N) < 0.5).astype(np.float64)
    z = rng.standard_normal(N)

    def why(values, covariates, kind):
        with pytest.raises(ss.Refused) as e:
            ss.null_fit(list(values), [list(c) for c in covariates], kind)
        return e.value.reason

    assert why(y, [np.ones(N)], "logistic") == ss.SKIP_CONSTANT
    assert why(y, [np.ones(N)], "linear") == ss.SKIP_CONSTANT
    few = np.full(N, np.nan)
    few[:4] = (0.0, 1.0, 1.0, 0.0)
    assert why(few, [z, z * z], "logistic") == ss.SKIP_FEW                  # n = 4 = q + 1
    more = few.copy()
    more[4] = 1.0
    assert ss.null_fit(list(more), [list(z)], "linear")["n"] == 5           # n = 5 > q + 1 = 3
    assert why(np.where(np.isnan(y), y, 1.0), [z], "logistic") == ss.SKIP_ONE_CLASS
    assert why(y, [z, 2.0 * z + 1.0], "logistic") == ss.SKIP_COLLINEAR
    assert why(z + y, [z, 2.0 * z + 1.0], "linear") == ss.SKIP_COLLINEAR
    assert why((z > 0.1).astype(np.float64), [z], "logistic") == ss.SKIP_SEPARATED


def test_the_engines_host_side_is_the_restatement(logistic_problems, linear_problems):
    """engine.score_host (numpy) against the restatement (plain loops): the same valid sets and n, rows, factor and
    residual sum of squares to 1e-8 -- two Newton iterations that both stop at a step of 1e-10 -- and the same
    refusals."""
    from scoary_amd import engine
    for kind, problems in (("logistic", logistic_problems), ("linear", linear_problems)):
        for N, c, y, cov, fit in problems[::3]:
            host = engine.score_host(y[None, :], cov, kind)
            rows, valid, packed = ss.plan_rows(fit, N)
            assert host["skipped"] == [None] and host["n"][0] == fit["n"]
            assert host["valid"][0].tolist() == [bool(v) for v in valid]
            assert np.allclose(host["rows"][0], np.array(rows), rtol=1e-8, atol=1e-9)
            assert np.allclose(host["chol"][0], np.array(packed), rtol=1e-8, atol=1e-9)
            assert np.all(host["rows"][0][:, ~host["valid"][0]] == 0.0)
            if kind == "linear":
                assert _rel(host["rss"][0], fit["rss"]) <= 1e-9
    rng = np.random.default_rng(16)
    N = 40
    y = (rng.random(N) < 0.5).astype(np.float64)
    z = rng.standard_normal(N)
    few = np.full(N, np.nan)
    few[:3] = (0.0, 1.0, 1.0)                                               # n = 3 = q + 1
    values = np.stack([y, few, np.ones(N), (z > 0.1).astype(np.float64)])
    host = engine.score_host(values, z[None, :], "logistic")
    assert host["skipped"] == [None, "few", "one_class", "separated"]
    assert not host["valid"][1:].any() and not host["rows"][1:].any()
    assert engine.score_host(values[:1], np.stack([z, 2.0 * z + 1.0]), "logistic")["skipped"] == ["collinear"]
    assert engine.score_host(values[:1], np.stack([z, np.ones(N)]), "linear")["skipped"] == ["constant"]
    assert list(engine.SCORE_SKIPS) == ["few", "constant", "one_class", "collinear", "separated"]
    for bad, text in (((values, np.zeros((9, N))), "9 covariates, at most 8"),
                      ((values * 2.0, None), "a binary trait is 0, 1 or nan"),
                      ((values, np.zeros((1, N + 1))), "covariates must be")):
        with pytest.raises(ValueError, match=text):
            engine.score_host(bad[0], bad[1], "logistic")
    with pytest.raises(ValueError, match="kind must be one of"):
        engine.score_host(values, None, "probit")
