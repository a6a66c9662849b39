"""k_score_observed (spec S24) on the GPU against the plain-Python restatement (score_spec.py) run on the plan's rows
as read back from the device: m, U, every b_j, Vg, the statistic, beta and se bit for bit, p within 1e-10 relative of
the restatement's tail at the device's own statistic -- at the shapes where the kernel can go wrong: one isolate, word
tails, one isolate past the LDS chunk and past two, one gene and one gene past a block, one and three traits with
valid sets of their own, every instance q = 1 .. 9, both kinds; genes of no, every and one isolate, of invalid
isolates only, equal to a 0 / 1 covariate, with the pad bits set; outputs that start as garbage; the refusals."""
import math

import numpy as np
import pytest

import score_spec as ss

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_SIZE = -1, -3
CHUNK = 512                                     # isolates of an LDS chunk of k_score_observed (kScoreChunk)
REL = 1e-10

# name: (N, G, T, covariates, kind)
SHAPES = {
    "n31": (31, 255, 3, 1, "logistic"),
    "n32": (32, 256, 1, 2, "linear"),
    "n33": (33, 257, 3, 3, "logistic"),
    "n64": (64, 70, 1, 4, "linear"),
    "n65": (65, 70, 3, 5, "logistic"),
    "n257": (257, 70, 1, 6, "linear"),
    "chunk": (CHUNK, 70, 1, 7, "logistic"),
    "chunk+1": (CHUNK + 1, 257, 3, 8, "logistic"),
    "chunk+1 linear": (CHUNK + 1, 70, 3, 8, "linear"),
    "two chunks+1": (2 * CHUNK + 1, 70, 1, 7, "linear"),
    "intercept logistic": (200, 70, 3, 0, "logistic"),
    "intercept linear": (200, 70, 1, 0, "linear"),
    "q2 linear": (65, 70, 1, 1, "linear"),
    "q5 logistic": (65, 1, 1, 4, "logistic"),
    "q9 linear": (200, 70, 1, 8, "linear"),
}


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _problem(name):
    """(genes [G, N] 0/1, values [T, N], covariates [c, N]) of a shape: covariate 0 is 0 / 1, every trait misses
    isolates of its own, a covariate misses one."""
    N, G, T, c, kind = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    cov = rng.standard_normal((c, N))
    if c:
        cov[0] = rng.random(N) < 0.4
        cov[c - 1, N // 3] = np.nan
    eta = (cov[1:].T @ rng.standard_normal(max(c - 1, 0)) / math.sqrt(c) if c > 1 else np.zeros(N))
    eta = np.nan_to_num(eta)
    values = np.empty((T, N))
    for t in range(T):
        if kind == "logistic":
            values[t] = rng.random(N) < 1.0 / (1.0 + np.exp(-(eta + 0.2 * t)))
        else:
            values[t] = eta + rng.standard_normal(N)
        values[t, rng.random(N) < 0.08] = np.nan
        values[t, t] = np.nan                    # isolate t is invalid in trait t
    genes = (rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))).astype(np.uint8)
    special = [np.zeros(N), np.ones(N), np.zeros(N), np.isnan(values[0]) | np.isnan(cov).any(axis=0),
               cov[0] == 1.0 if c else np.zeros(N)]
    valid0 = np.flatnonzero(~special[3])
    special[2][valid0[-1]] = 1                   # one isolate: the last valid one of trait 0
    if G >= 10:
        for g, row in enumerate(special):
            genes[G - 1 - g] = row               # at the end: the last block's tail holds them
    return genes, values, cov


def _expected(plan_rows, valid, chol, rss, genes, kind):
    """Per trait the restatement on the rows read back: the sums of every gene as sequential numpy sums (+0.0 for a
    non-carrier: the same bits as the walk over the carriers, which the first genes and the special ones are held to
    by score_spec.gene_sums itself), then score_spec.finish."""
    T, rows_n, N = plan_rows.shape
    G = len(genes)
    out = []
    for t in range(T):
        on = (genes != 0) & valid[t][None, :]
        m = on.sum(axis=1)
        sums = np.stack([np.add.accumulate(np.where(on, plan_rows[t, j][None, :], 0.0), axis=1)[:, -1]
                         for j in range(rows_n)], axis=1)                                  # [G, q + 1]
        rows = [r.tolist() for r in plan_rows[t]]
        vbits = valid[t].astype(int).tolist()
        for g in list(range(min(G, 6))) + list(range(max(G - 6, 0), G)):
            mm, U, b = ss.gene_sums(genes[g].tolist(), rows, vbits)
            assert mm == m[g] and _bits([U] + b).tolist() == _bits(sums[g]).tolist()
        n = int(valid[t].sum())
        packed = chol[t].tolist()
        out.append([ss.finish(int(m[g]), float(sums[g, 0]), sums[g, 1:].tolist(), n, packed, kind, float(rss[t]))
                    for g in range(G)])
    return out


def _compare(res, want, kind, name):
    stat = "t" if kind == "linear" else "stat"
    tested = 0
    for t, per_gene in enumerate(want):
        for g, w in enumerate(per_gene):
            where = (name, t, g)
            assert int(res["m"][t, g]) == w["m"], where
            assert _bits(res["U"][t, g]) == _bits(w["U"]), where
            assert _bits(res["b"][t, g]).tolist() == _bits(w["b"]).tolist(), where
            assert _bits(res["Vg"][t, g]) == _bits(w["Vg"]), where
            for key, field in ((stat, "stat"), ("beta", "beta"), ("se", "se")):
                assert _bits(res[key][t, g]) == _bits(w[field]), where + (key, float(res[key][t, g]), w[field])
            p = float(res["p"][t, g])
            if not w["testable"]:
                assert p == 1.0 and float(res[stat][t, g]) == 0.0, where
                continue
            tested += 1
            ref = ss.p_of(kind, float(res[stat][t, g]), w["df"])
            if ref > 1e-290:
                assert abs(p - ref) <= REL * ref, where + (p, float(ref))
            else:
                assert 0.0 <= p <= 1e-289, where
    return tested


_CACHE = {}


def _case(eng, name):
    if name not in _CACHE:
        N, G, T, c, kind = SHAPES[name]
        genes, values, cov = _problem(name)
        gm = eng.pack_dense(genes)
        plan = eng.score_plan(values, cov, kind)
        res = {k: v.cpu().numpy() for k, v in eng.score(gm, plan).items()}
        _CACHE[name] = (genes, values, cov, gm, plan, res)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_score_matches_the_restatement(eng, name):
    N, G, T, c, kind = SHAPES[name]
    genes, values, cov, gm, plan, res = _case(eng, name)
    assert plan.q == c + 1 and plan.skipped == [None] * T, plan.skipped
    assert len({tuple(v) for v in plan.valid_host.tolist()}) == T           # valid sets of their own
    rows = plan.rows.cpu().numpy()
    assert rows.shape == (T, c + 2, N) and np.all(rows.transpose(0, 2, 1)[~plan.valid_host] == 0.0)
    want = _expected(rows, plan.valid_host, plan.chol.cpu().numpy(), plan.rss.cpu().numpy(), genes, kind)
    tested = _compare(res, want, kind, name)
    assert tested >= T * max(1, (G - 5) // 2) or G == 1
    # the special genes (the last rows of the matrix): none, every, one, invalid only, the 0 / 1 covariate
    stat = "t" if kind == "linear" else "stat"
    for k in range(5 if G >= 10 else 0):
        g = G - 1 - k
        if k == 2:
            assert res["m"][0, g] == 1 and want[0][g]["testable"]
        elif k == 4 and c:
            for t in range(T):
                assert 0 < res["m"][t, g] < plan.n[t] and res["Vg"][t, g] <= ss.VG_CUT * res["b"][t, g, 0]
                assert res["p"][t, g] == 1.0 and res[stat][t, g] == 0.0
        elif k != 4:
            assert res["m"][0, g] == (0, plan.n[0], 1, 0)[k] and res["p"][0, g] == 1.0


def test_one_isolate_and_rows_that_are_not_zero_outside_the_valid_set(eng):
    """Plans made by hand (score_plan_of): N = 1 with its isolate valid, and N = 70 with garbage in the rows of the
    invalid isolates, which the validity bits keep out of every sum; q = 1 and q = 3, both kinds, G = 1 and 70."""
    rng = np.random.default_rng(24)
    for N, G, q in ((1, 1, 1), (70, 70, 3), (1, 3, 2)):
        for kind in ("logistic", "linear"):
            T = 2
            valid = rng.random((T, N)) < 0.8
            valid[:, 0] = True
            rows = rng.standard_normal((T, q + 1, N))
            rows[:, 1] = np.abs(rows[:, 1]) + 0.1                            # weights
            A = rng.standard_normal((T, q, q + 3))
            chol = np.stack([np.linalg.cholesky(a @ a.T + np.eye(q))[np.tril_indices(q)] for a in A])
            host = dict(rows=rows, valid=valid, chol=chol, rss=np.abs(rng.standard_normal(T)) * N + 50.0,
                        n=valid.sum(axis=1), coef=np.zeros((T, q)), skipped=[None] * T)
            genes = (rng.random((G, N)) < 0.6).astype(np.uint8)
            genes[0] = 1
            plan = eng.score_plan_of(host, kind)
            res = {k: v.cpu().numpy() for k, v in eng.score(eng.pack_dense(genes), plan).items()}
            want = _expected(plan.rows.cpu().numpy(), valid, chol, host["rss"], genes, kind)
            _compare(res, want, kind, "by hand N=%d q=%d %s" % (N, q, kind))
            assert np.array_equal(res["m"][:, 0], valid.sum(axis=1))


LADDER_DF = (0, 1, 2, 3, 38, 39, 40, 41, 2000)
LADDER_CELLS = 120                               # (trait, gene) cells of a ladder, at the least


def _ladder(df):
    """A linear plan made by hand whose t statistics are a ladder: q = 1, every weight 1, chol = [sqrt(n)], every
    isolate valid, n = df + 2; gene g is the single carrier g, so U = r_g and Vg = 1 - 1/n, over G = min(n - 1, 60)
    genes and as many traits as give 120 cells (n = 3 has two genes).  Cell k of K (trait by trait) aims at
    |t| = 1e-8 (t_top / 1e-8)^(k / (K - 1)), a geometric ladder, through r = +-sqrt(y rss Vg) with
    y = t^2 / (df + t^2) = U^2 / (Vg rss), odd cells negative; t_top^2 = df min(10^(600 / df), 2^50) is where the
    tail is 1e-300, or as close to rss as a double lets U^2 / Vg come (rss1 is then a few ulps of rss: at df < 39
    the ladder ends above 1e-280).  rss differs from trait to trait.  The last two genes of trait 0 have
    U^2 / Vg = 4 rss, one with U > 0 and one with U < 0: rss1 < 0, t = +-inf, p = 0.
    Returns (host dict for score_plan_of, genes)."""
    n = df + 2
    G = min(n - 1, 60)
    T = -(-LADDER_CELLS // G)
    K = T * G
    rows = np.zeros((T, 2, n))
    rows[:, 1] = 1.0
    rss = 1.0 + 0.37 * np.arange(T)
    vg = 1.0 - (1.0 / math.sqrt(n)) ** 2
    top2 = max(df, 1) * min(10.0 ** min(600.0 / max(df, 1), 300.0), 2.0 ** 50)
    for k in range(K):
        t, g = divmod(k, G)
        t2 = (1e-8 * (math.sqrt(top2) / 1e-8) ** (k / (K - 1.0))) ** 2
        y = t2 / (max(df, 1) + t2)
        if t == 0 and g >= G - 2:
            y = 4.0
        rows[t, 0, g] = (-1.0 if (k if y < 4.0 else g) % 2 else 1.0) * math.sqrt(y * rss[t] * vg)
    host = dict(rows=rows, valid=np.ones((T, n), dtype=bool), chol=np.full((T, 1), math.sqrt(n)), rss=rss,
                n=np.full(T, n), coef=np.zeros((T, 1)), skipped=[None] * T)
    return host, np.eye(n, dtype=np.uint8)[:G]


@pytest.mark.parametrize("df", LADDER_DF)
def test_student_tail_ladder(eng, df):
    """t_tail at the degrees of freedom the other shapes do not reach: df = 1, 2, 3 (lgamma at 0.5 to 1.5, the
    branch switch of the fraction at x < 1/2), 38 to 41 (a = 19 to 20.5: lgamma gives way to the series at a = 20),
    2000, and df = 0 (every gene untestable); |t| from 1e-8, where the tail is next to 1, to tails below 1e-280
    where df allows it, half of them negative, and t = +-inf.  Held as every other shape is: the sums and the
    statistic bit for bit, p within 1e-10 relative of mpmath at 50 digits at the device's own t."""
    host, genes = _ladder(df)
    T, G = len(host["rss"]), len(genes)
    plan = eng.score_plan_of(host, "linear")
    res = {k: v.cpu().numpy() for k, v in eng.score(eng.pack_dense(genes), plan).items()}
    assert np.array_equal(plan.rows.cpu().numpy(), host["rows"])
    want = _expected(host["rows"], host["valid"], host["chol"], host["rss"], genes, "linear")
    tested = _compare(res, want, "linear", "ladder df=%d" % df)
    if df == 0:
        assert tested == 0 and G == 1 and np.all(res["p"] == 1.0) and not res["t"].any()
    else:
        assert tested == T * G and want[0][0]["df"] == df
        _ladder_reaches(res["t"], res["p"], df)


def _ladder_reaches(t, p, df):
    """What the ladder is there for, on the statistics and tails [T, G] as they came out: both infinite statistics,
    half of the finite ones negative, |t| from below 2e-8 (a tail next to 1) to the top, tails below 1e-280 where a
    double lets rss1 get small enough for them (df >= 38; at df = 1, 2, 3 the top is |t| above 1e7)."""
    G = t.shape[1]
    assert sorted(t[0, G - 2:].tolist()) == [-math.inf, math.inf] and not p[0, G - 2:].any()
    finite = np.isfinite(t)
    assert finite.sum() >= t.size - 4                                # a top rung may round to rss1 <= 0
    assert 0.45 <= (t[finite] < 0).mean() <= 0.55
    assert 0.0 < np.abs(t[finite]).min() < 2e-8 and 1.0 - 1e-7 < p[finite].max() < 1.0
    assert (p[finite] < 1e-280).any() if df >= 38 else np.abs(t[finite]).max() > 1e7
    assert np.unique(np.abs(t[finite])).size >= finite.sum() - 2


def test_a_skipped_trait_has_no_testable_gene(eng):
    rng = np.random.default_rng(25)
    N, G = 40, 30
    z = rng.standard_normal(N)
    values = np.stack([(rng.random(N) < 0.5), z > 0.1, np.ones(N)]).astype(np.float64)
    genes = (rng.random((G, N)) < 0.5).astype(np.uint8)
    plan = eng.score_plan(values, z[None, :], "logistic")
    assert plan.skipped == [None, "separated", "one_class"]
    res = {k: v.cpu().numpy() for k, v in eng.score(eng.pack_dense(genes), plan).items()}
    assert (res["p"][0] < 1.0).any()
    for t in (1, 2):
        assert not res["m"][t].any() and np.all(res["p"][t] == 1.0) and not res["stat"][t].any()
        assert not res["U"][t].any() and not res["b"][t].any() and not res["Vg"][t].any()


@pytest.mark.parametrize("name", ["n33", "chunk+1 linear", "n64"])
def test_pad_bits_past_the_last_isolate_do_not_enter(eng, name):
    """Every bit of the tiled matrix at and past isolate N set: the results keep their bits."""
    from scoary_amd.engine import GeneMatrix
    N, G, T, c, kind = SHAPES[name]
    genes, values, cov, gm, plan, res = _case(eng, name)
    tiled = gm.tiled.clone()
    words = tiled.shape[0] * 4
    for w in range(N // 32, words):
        fill = -1 if 32 * w >= N else -(1 << (N - 32 * w))           # as int32: the bits from N - 32 w up
        tiled[w // 4, :, w % 4] |= fill
    again = {k: v.cpu().numpy() for k, v in eng.score(GeneMatrix(tiled, G, N), plan).items()}
    for k in res:
        assert np.array_equal(res[k].view(np.uint64 if res[k].dtype == np.float64 else res[k].dtype),
                              again[k].view(np.uint64 if res[k].dtype == np.float64 else res[k].dtype)), k


def _raw(eng, gm, plan, G, T, N, q, linear, outs, ptrs=None):
    ptr = eng._ptr
    a = [ptr(gm.tiled), ptr(plan.rows), ptr(plan.valid), ptr(plan.chol), ptr(plan.rss)]
    if ptrs:
        a = [None if k in ptrs else x for k, x in enumerate(a)]
    return eng.lib.scoary_score(eng.h, *a, G, T, N, q, linear, *(ptr(o) for o in outs), eng._stream())


def test_stale_outputs_and_refusals(eng):
    """Outputs that start as garbage are overwritten for every (trait, gene) and untouched behind; a refusal is a
    status code with a message and launches nothing."""
    import torch
    name = "n33"
    N, G, T, c, kind = SHAPES[name]
    genes, values, cov, gm, plan, res = _case(eng, name)
    q, tail = c + 1, 64

    def garbage():
        outs = [torch.full((T * G + tail,), 77, dtype=torch.int32, device=eng.device)]
        outs += [torch.full((T * G * (q if k == 1 else 1) + tail,), float("nan"), dtype=torch.float64, device=eng.device)
                 for k in range(7)]
        return outs

    outs = garbage()
    assert _raw(eng, gm, plan, G, T, N, q, 0, outs) == 0
    torch.cuda.synchronize()
    for o, key in zip(outs, ("m", "U", "b", "Vg", "stat", "beta", "se", "p")):
        got = o.cpu().numpy()
        kind_ = np.uint64 if got.dtype == np.float64 else got.dtype
        assert np.array_equal(got[:-tail].view(kind_), res[key].ravel().view(kind_)), key
        assert bool((got[-tail:] == 77).all()) if key == "m" else bool(np.isnan(got[-tail:]).all()), key

    assert eng.score_max_covariates() == 8
    outs = garbage()
    for args, code in (((G, T, N, 0, 0), ERR_SIZE), ((G, T, N, 10, 0), ERR_SIZE), ((G, 65536, N, q, 0), ERR_SIZE),
                       (((1 << 31) - 256, T, N, q, 0), ERR_SIZE), ((G, T, (1 << 31) - 512, q, 0), ERR_SIZE),
                       ((0, T, N, q, 0), ERR_ARG), ((G, 0, N, q, 0), ERR_ARG), ((G, T, 0, q, 0), ERR_ARG),
                       ((G, T, N, q, 2), ERR_ARG), ((G, T, N, q, -1), ERR_ARG)):
        assert _raw(eng, gm, plan, *args, outs) == code, args
        assert b"scoary_score" in eng.lib.scoary_last_error(eng.h)
    for missing in range(4):
        assert _raw(eng, gm, plan, G, T, N, q, 0, outs, ptrs=(missing,)) == ERR_ARG
    assert _raw(eng, gm, plan, G, T, N, q, 1, outs, ptrs=(4,)) == ERR_ARG      # the linear kind reads d_rss
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        got = o.cpu().numpy()
        assert bool((got == 77).all()) if k == 0 else bool(np.isnan(got).all())
    assert _raw(eng, gm, plan, G, T, N, q, 0, outs, ptrs=(4,)) == 0            # the logistic kind does not
    torch.cuda.synchronize()
    assert np.array_equal(outs[7].cpu().numpy()[:-tail].view(np.uint64), res["p"].ravel().view(np.uint64))
    with pytest.raises(ValueError, match="the plan has 33 isolates, the gene matrix 64"):
        eng.score(_case(eng, "n64")[3], plan)
    with pytest.raises(ValueError, match="9 covariates, at most 8"):
        eng.score_plan(values, np.zeros((9, N)), kind)
