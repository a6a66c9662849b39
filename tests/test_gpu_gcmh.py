"""The generalized CMH kernels (spec S21) on the GPU against the plain-Python restatement (gcmh_spec.py):
k_gcmh_observed's tables, moments, form and statistic bit for bit, and k_gcmh_permute's exceedance counts twice over --
from the code rows read back and from the seed alone -- at the shapes where they can go wrong: one isolate, word and
stage tails, 1, 2, 9 and 1024 strata (some empty), the chunk boundary of the isolates, the largest matrix with strata
of 16 319 and 1 isolates, 1 to 8 classes and an empty one, every rank-deficient family, genes that are absent from or
fill a stratum, one batch against two, counts that start above zero, exact ties."""
import numpy as np
import pytest

import categorical_spec as cs
import gcmh_spec as gs
from cmh_homog_spec import chi2_sf

pytestmark = pytest.mark.gpu
SEED = 0x5EED6C31
ERR_SIZE = -3
CHUNK = 2432                                   # isolates of a chunk of k_gcmh_permute (kCatChunk)
# name: (N, S, G, P, batches)
SHAPES = {"n1": (1, 1, 1, 1, 1), "n9": (9, 1, 70, 500, 1), "n21": (21, 2, 70, 500, 1), "n33": (33, 9, 255, 63, 1),
          "n64": (64, 2, 256, 130, 2), "n65": (65, 9, 257, 65, 1), "families": (40, 6, 70, 64, 1),
          "chunk2432": (CHUNK, 1024, 70, 3, 1), "chunk2433": (CHUNK + 1, 2, 70, 3, 1),
          "largest": (cs.MAX_ISOLATES, 2, 70, 3, 1)}


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _shape(name):
    """(genes [G, N] 0/1, codes [T, N], strata [N]) of a shape."""
    N, S, G, _P, _b = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "largest":
        strata = np.zeros(N, dtype=np.int64)
        strata[N // 3] = 1                     # strata of 16 319 and 1 isolates
    elif name == "families":
        strata = np.repeat(np.arange(6), [10, 10, 10, 8, 1, 1])
    elif name == "n21":
        strata = np.repeat(np.arange(2), [10, 11])
    else:
        strata = rng.integers(0, S, N)
        strata[N - 1] = S - 1                  # the last stratum is in use; at S = 1024 many others are empty
    traits = []
    if name in ("n9", "n21"):                  # the tie trait: classes (3, 3, 3) in every stratum, the rest missing
        tie = np.zeros(N, dtype=np.int64)
        for s in range(S):
            tie[np.flatnonzero(strata == s)[:9]] = np.repeat(np.arange(1, 4), 3)[:min(9, int((strata == s).sum()))]
        traits.append(tie)
    k3 = rng.integers(0, 4, N)                 # K = 3 with missing isolates
    k8 = rng.integers(1, 9, N)                 # K = 8, no missing isolate
    traits += [k3, k8]
    if name == "families":
        lo, hi = strata < 2, (strata == 2) | (strata == 3)
        disjoint = np.where(lo, rng.integers(1, 3, N), np.where(hi, rng.integers(3, 5, N), 0))
        joined = disjoint.copy()
        joined[30], joined[31] = 2, 2          # stratum 3 now holds classes of both groups
        only3 = np.where(strata < 3, rng.integers(1, 3, N), 0)             # class 3 lives in stratum 3 alone
        only3[30:38] = [1, 3, 1, 3, 1, 3, 3, 1]
        traits += [disjoint, joined, only3]
    if N <= 1000:
        k1 = (rng.random(N) < 0.8).astype(np.int64)                       # K = 1: untestable
        k2 = rng.integers(1, 3, N)
        k5 = rng.integers(0, 6, N)
        gap = rng.choice([0, 1, 3], N)                                    # class 2 is empty
        traits += [k1, k2, k5, gap, np.zeros(N, dtype=np.int64)]          # and a trait without a label
    codes = np.stack(traits).astype(np.int64)
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    if G > 9:
        genes[1] = 0                           # m_s = 0 everywhere
        genes[2] = 1                           # m_s = n_s everywhere
        genes[3] = 0
        genes[3, N - 1] = 1                    # one isolate, the last
        genes[4] = 1
        genes[4, 0] = 0
        edge = 3 if name == "families" else strata[N - 1]
        genes[8, strata == edge] = 0           # absent from one stratum,
        genes[9, strata == edge] = 1           # filling it
        genes[6] = codes[0] == 0               # carried only by isolates without a label (first trait)
        genes[7] = codes[1] == 1               # equal to a class of the second trait
    return genes, codes, strata


def _tables(genes, rows, K=8):
    """a[.., g, k] of 0/1 genes [G, N] against code rows [.., N] (ints): exact, in numpy (counts far below 2^24)."""
    onehot = (np.asarray(rows)[..., None] == np.arange(1, K + 1)).astype(np.float32)      # [.., N, K]
    parts = [np.einsum("gn,...nk->...gk", genes[g0:g0 + 8192].astype(np.float32), onehot, optimize=True)
             for g0 in range(0, len(genes), 8192)]
    return np.rint(np.concatenate(parts, axis=-2)).astype(np.int64)


def _spec(genes, row, strata, S):
    """The restatement of one trait over all genes: dict(a, ms, m, E, form, df, q, thr)."""
    row = np.asarray(row)
    nsk = gs.margins(row.tolist(), strata.tolist(), S)
    member = ((strata[:, None] == np.arange(S)) & (row[:, None] != 0)).astype(np.float32)          # [N, S]
    ms = np.rint(genes.astype(np.float32) @ member).astype(np.int64)
    a = _tables(genes, row)
    E, V = gs.moments_many(ms, nsk)
    form, df = gs.factor_many(E, V, max(gs.klast(nsk) - 1, 0))
    q = gs.q_many(a, form)
    return dict(nsk=nsk, a=a, ms=ms, m=ms.sum(axis=1), E=E, form=form, df=df, q=q, thr=q * gs.ONE_MINUS_TAU)


_CACHE = {}


def _case(eng, name):
    """Everything one shape needs, computed once: the device results, the rows and the restatement."""
    import torch
    if name in _CACHE:
        return _CACHE[name]
    genes, codes, strata = _shape(name)
    N, S, G, P, batches = SHAPES[name]
    T = codes.shape[0]
    gm = eng.pack_dense(genes)
    plan = eng.gcmh_plan(codes, strata)
    assert plan.S == S and plan.T == T
    obs = eng.gcmh(gm, plan)
    res = {k: v.cpu().numpy() for k, v in obs.items()}
    rows = eng.gcmh_rows(plan, 0, P, SEED).cpu().numpy()
    budget = (8 << 30) if batches == 1 else 2 * (2 * 64 * T * N)           # two stages of 64 permutations per batch
    assert -(-P // eng.categorical_batch(T, N, P, budget)) == batches
    r = eng.gcmh_permute(gm, plan, obs, P, SEED, budget_bytes=budget).cpu().numpy()
    r5 = torch.full((T, G), 5, dtype=torch.int32, device=eng.device)      # one call on the rows read back, from 5
    eng.permute_gcmh(gm, plan, obs, torch.from_numpy(rows).to(eng.device), r5)
    spec_rows = np.array([[gs.perm_row(SEED, t, pi, codes[t].tolist(), strata.tolist(), S) for pi in range(P)]
                          for t in range(T)])
    spec = [_spec(genes, codes[t], strata, S) for t in range(T)]
    _CACHE[name] = dict(genes=genes, codes=codes, strata=strata, plan=plan, res=res, rows=rows, r=r,
                        r5=r5.cpu().numpy(), spec_rows=spec_rows, spec=spec)
    return _CACHE[name]


CASES = tuple(SHAPES)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", CASES)
def test_observed_tables_moments_form_and_statistic(eng, name):
    c = _case(eng, name)
    genes, codes, strata, res, plan = c["genes"], c["codes"], c["strata"], c["res"], c["plan"]
    N, S, G, _P, _b = SHAPES[name]
    kinds, worst_p = set(), 0.0
    for t in range(codes.shape[0]):
        sp = c["spec"][t]
        assert plan.nsk_host[t].tolist() == sp["nsk"]
        for g in sorted({0, min(3, G - 1), G - 1}):                      # the numpy route is the scalar restatement's
            a, ms = gs.counts(genes[g].tolist(), codes[t].tolist(), strata.tolist(), S)
            st = gs.statistic(a, ms, sp["nsk"])
            assert (a, ms) == (sp["a"][g].tolist(), sp["ms"][g].tolist())
            assert (st["E"], st["form"], st["df"], st["q"]) == (sp["E"][g].tolist(), sp["form"][g].tolist(),
                                                                sp["df"][g], sp["q"][g])
        assert np.array_equal(res["a"][t], sp["a"]) and np.array_equal(res["m"][t], sp["m"])
        assert np.array_equal(res["df"][t], sp["df"])
        for key, want in (("e", sp["E"]), ("form", sp["form"]), ("q", sp["q"]), ("thr", sp["thr"])):
            assert np.array_equal(_bits(res[key][t]), _bits(want)), (name, t, key)               # bit for bit
        for g in range(G):
            df = int(sp["df"][g])
            kinds.add(df)
            if df == 0:
                assert (res["q"][t, g], res["p"][t, g], res["thr"][t, g]) == (0.0, 1.0, 0.0)
                assert not res["form"][t, g, 7:].any()
                continue
            p = chi2_sf(float(sp["q"][g]), df)
            if p > 1e-290:
                assert abs(res["p"][t, g] - p) <= 1e-10 * p, (t, g, res["p"][t, g], p)
                worst_p = max(worst_p, abs(res["p"][t, g] - p) / p)
    print("%s: df values %s, worst relative error of p %.3g" % (name, sorted(kinds), worst_p))
    assert 0 in kinds and (N == 1 or max(kinds) >= 2)


def test_the_families_case_meets_every_rank_deficient_family(eng):
    c = _case(eng, "families")
    codes, strata = c["codes"], c["strata"]
    T = codes.shape[0]
    disjoint, joined, only3 = 2, 3, 4
    df = [c["spec"][t]["df"] for t in range(T)]
    assert sorted(set(codes[disjoint])) == [0, 1, 2, 3, 4] and df[disjoint].max() == 2       # two groups of two classes
    assert df[joined].max() == 3                                                           # joined by stratum 3
    # class 3 is present only in stratum 3: a gene that is absent from it or fills it sees two classes
    assert df[only3][8] == df[only3][9] == 1 and df[only3].max() == 2
    assert (np.bincount(strata) == 1).sum() == 2                                           # strata of one isolate
    ms = c["spec"][0]["ms"]
    assert (ms == 0).any() and (ms[2] == np.array(gs.margins(codes[0].tolist(), strata.tolist(), 6)).sum(axis=1)).all()
    for t in range(T):
        assert np.array_equal(c["res"]["df"][t], df[t])


@pytest.mark.parametrize("name", CASES)
def test_rows_are_the_shuffle_of_the_seed_within_the_strata(eng, name):
    c = _case(eng, name)
    assert np.array_equal(c["rows"], c["spec_rows"])
    S = SHAPES[name][1]
    for t in range(c["codes"].shape[0]):
        want = c["spec"][t]["nsk"]
        for pi in (0, c["rows"].shape[1] - 1):
            assert gs.margins(c["rows"][t, pi].tolist(), c["strata"].tolist(), S) == want


@pytest.mark.parametrize("name", CASES)
def test_exceedance_counts_from_the_rows_and_from_the_seed(eng, name):
    c = _case(eng, name)
    genes, codes = c["genes"], c["codes"]
    P = SHAPES[name][3]
    for t in range(codes.shape[0]):
        sp = c["spec"][t]
        from_rows = (gs.q_many(_tables(genes, c["rows"][t]), sp["form"]) >= sp["thr"]).sum(axis=0)
        from_seed = (gs.q_many(_tables(genes, c["spec_rows"][t]), sp["form"]) >= sp["thr"]).sum(axis=0)
        for g in sorted({0, len(genes) - 1}):                            # the numpy count is the scalar restatement's
            n = sum(1 for row in c["spec_rows"][t].tolist()
                    if gs.q_of(gs.counts(genes[g].tolist(), row, c["strata"].tolist(), SHAPES[name][1])[0],
                               sp["form"][g].tolist()) >= sp["thr"][g])
            assert from_seed[g] == n
        assert np.array_equal(c["r"][t], from_rows), (name, t)
        assert np.array_equal(c["r"][t], from_seed), (name, t)
        assert np.array_equal(c["r5"][t], from_rows + 5), (name, t)
        assert (c["r"][t][sp["df"] == 0] == P).all()                     # an untestable gene: r = P, by itself


@pytest.mark.parametrize("N", [33, CHUNK + 1])
def test_blocks_that_walk_several_gene_groups(eng, N):
    """More gene groups than a launch has ranges: a block walks several groups -- with one chunk of isolates on the
    rows it loaded once, with two on rows it loads again for every group."""
    rng = np.random.default_rng(N)
    G, T, P, S = 64 * 520 + 6, 2, 3, 3
    genes = (rng.random((G, N)) < rng.uniform(0.0, 1.0, (G, 1))).astype(np.uint8)
    codes = np.stack([rng.integers(0, 4, N), rng.integers(1, 9, N)])
    strata = rng.integers(0, S, N)
    strata[0] = S - 1
    gm = eng.pack_dense(genes)
    plan = eng.gcmh_plan(codes, strata)
    obs = eng.gcmh(gm, plan)
    r = eng.gcmh_permute(gm, plan, obs, P, SEED).cpu().numpy()
    for t in range(T):
        sp = _spec(genes, codes[t], strata, S)
        rows = np.array([gs.perm_row(SEED, t, pi, codes[t].tolist(), strata.tolist(), S) for pi in range(P)])
        assert np.array_equal(_bits(obs["form"][t].cpu().numpy()), _bits(sp["form"]))
        assert np.array_equal(_bits(obs["thr"][t].cpu().numpy()), _bits(sp["thr"]))
        assert np.array_equal(r[t], (gs.q_many(_tables(genes, rows), sp["form"]) >= sp["thr"]).sum(axis=0)), t


@pytest.mark.parametrize("name", ["n9", "n21"])
def test_the_tie_trait_meets_exact_ties_between_distinct_tables_and_counts_them_all(eng, name):
    c = _case(eng, name)
    genes, codes, strata = c["genes"], c["codes"], c["strata"]
    S = SHAPES[name][1]
    sp = c["spec"][0]
    assert all(row[:3] == [3, 3, 3] for row in sp["nsk"])
    nc = gs.klast(sp["nsk"]) - 1
    ties = 0
    for g in range(len(genes)):
        if sp["df"][g] == 0:
            continue
        a_obs, ms = gs.counts(genes[g].tolist(), codes[0].tolist(), strata.tolist(), S)
        E, V = gs.moments_exact(ms, sp["nsk"], range(nc))
        L, piv, _rel = gs.factor_exact(V)
        q_obs = gs.q_factored_exact([a_obs[k] - E[k] for k in range(nc)], L, piv)[0]
        exact = 0
        for a in _tables(genes[g:g + 1], c["spec_rows"][0])[:, 0].tolist():
            q = gs.q_factored_exact([a[k] - E[k] for k in range(nc)], L, piv)[0]
            exact += q >= q_obs
            ties += q == q_obs and a != a_obs
        assert c["r"][0, g] == exact, g                                  # the rational rule itself, at this input
    print("%s: %d permuted tables tie with a different observed one" % (name, ties))
    assert ties > 100


def test_one_stratum_gives_the_rows_and_the_counts_of_the_chi_square_step(eng):
    """S = 1: the rows are categorical_rows' and r is scoary_permute_categorical's, at an input where the restatement
    finds no permuted table inside the band below an observed Q."""
    rng = np.random.default_rng(20)
    G, N, P = 70, 40, 200
    genes = (rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))).astype(np.uint8)
    codes = np.stack([rng.integers(0, 4, N), rng.integers(1, 6, N)])
    strata = np.zeros(N, dtype=np.int64)
    gm = eng.pack_dense(genes)
    plan, cplan = eng.gcmh_plan(codes, strata), eng.categorical_plan(codes)
    obs, cobs = eng.gcmh(gm, plan), eng.categorical(gm, cplan)
    rows = eng.gcmh_rows(plan, 0, P, SEED)
    assert np.array_equal(rows.cpu().numpy(), eng.categorical_rows(cplan, 0, P, SEED).cpu().numpy())
    r = eng.gcmh_permute(gm, plan, obs, P, SEED).cpu().numpy()
    rc = eng.categorical_permute(gm, cplan, cobs["a"], P, SEED).cpu().numpy()
    for t in range(2):
        sp = _spec(genes, codes[t], strata, 1)
        nk = cs.sizes(codes[t].tolist(), 8)
        a_perm, a_obs = _tables(genes, rows[t].cpu().numpy()), sp["a"]
        w = np.array(cs.weights(nk), dtype=np.int64)
        exact = ((a_perm ** 2) @ w >= ((a_obs ** 2) @ w)[None])          # S20's rule in integers
        banded = gs.q_many(a_perm, sp["form"]) >= sp["thr"]
        testable = (sp["df"] > 0)[None]
        assert np.array_equal(exact & testable, banded & testable)      # no pair inside the band
        n = sum(nk)
        x2 = cobs["x2"][t].cpu().numpy()
        assert np.allclose(obs["q"][t].cpu().numpy(), x2 * (n - 1) / n, rtol=1e-12, atol=0)
        assert np.array_equal(r[t], rc[t])


def test_sizes_past_the_limits_are_refused_with_nothing_written(eng):
    import torch
    G, T, N, P, S = 10, 1, 40, 5, 2
    gm = eng.pack_dense(np.ones((G, N), dtype=np.uint8))
    plan = eng.gcmh_plan(np.ones((T, N), dtype=np.int64), np.arange(N) % S)
    pat = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=eng.device)        # noqa: E731
    a, m, df, r = pat((T, G, 8), torch.int32), pat((T, G), torch.int32), pat((T, G), torch.int32), pat((T, G), torch.int32)
    e, form = pat((T, G, 8), torch.float64), pat((T, G, 35), torch.float64)
    q, p, thr = (pat((T, G), torch.float64) for _ in range(3))
    rows = torch.zeros((T, P, N), dtype=torch.int16, device=eng.device)
    scratch = eng._cmh_scratch(N)
    ptr = eng._ptr
    big = eng.ranksum_max_isolates() + 1
    assert int(eng.lib.scoary_gcmh_form_doubles()) == 35 == gs.FORM

    def observed(g, t, n, K, s):
        return eng.lib.scoary_gcmh(eng.h, ptr(gm.tiled), ptr(plan.codes), ptr(plan.nk), ptr(plan.nsk), ptr(plan.strata),
                                   ptr(plan.members), g, t, n, K, s, ptr(a), ptr(m), ptr(e), ptr(form), ptr(q), ptr(df),
                                   ptr(p), ptr(thr), ptr(scratch), eng._stream())

    def permute(g, t, n, pp):
        return eng.lib.scoary_permute_gcmh(eng.h, ptr(gm.tiled), ptr(rows), ptr(form), ptr(thr), ptr(plan.nk), g, t, n,
                                           pp, ptr(r), eng._stream())
    for g, t, n, K, s in ((G, T, N, 9, S), (G, T, N, 0, S), (G, T, big, 3, S), (G, T, N, 3, eng.strata_max()[0] + 1),
                          (G, 65536, N, 3, S), (1 << 31, T, N, 3, S)):
        assert observed(g, t, n, K, s) == ERR_SIZE, (g, t, n, K, s)
    for g, t, n, pp in ((G, T, big, P), (G, T, N, 1 << 31), (G, 65536, N, P), (1 << 31, T, N, P)):
        assert permute(g, t, n, pp) == ERR_SIZE, (g, t, n, pp)
    torch.cuda.synchronize()
    for x in (a, m, df, r, e, form, q, p, thr):
        assert bool((x == 77).all())
    with pytest.raises(ValueError, match="a code is 0 .missing. or a class 1 .. 8"):
        eng.gcmh_plan(np.full((1, 4), 9), np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError, match="strata, the kernels take"):
        eng.gcmh_plan(np.ones((1, 4), dtype=np.int64), np.array([0, 1, 2, eng.strata_max()[0]]))
    with pytest.raises(ValueError, match="must not be negative"):
        eng.gcmh_plan(np.ones((1, 4), dtype=np.int64), np.array([0, 1, -1, 0]))


def test_a_row_with_codes_outside_the_classes_stays_inside_the_buffers(eng):
    """Codes that are none of the trait's (negative, past 8) match no plane: wrong numbers, the neighbours untouched."""
    import torch
    genes, codes, strata = _shape("n33")
    gm = eng.pack_dense(genes)
    plan = eng.gcmh_plan(codes[:1], strata)
    obs = eng.gcmh(gm, plan)
    rows = torch.tensor([-32768, 32767, 9, -1, 8] * 33, dtype=torch.int16, device=eng.device)[:2 * 33].reshape(1, 2, 33)
    guard = torch.full((3, len(genes)), 9, dtype=torch.int32, device=eng.device)
    eng.permute_gcmh(gm, plan, obs, rows.contiguous(), guard[1:2])
    torch.cuda.synchronize()
    got = guard.cpu().numpy()
    assert (got[0] == 9).all() and (got[2] == 9).all() and ((got[1] >= 9) & (got[1] <= 11)).all()
