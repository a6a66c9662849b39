"""The categorical kernels (spec S20) on the GPU against the plain-Python restatement (categorical_spec.py):
k_cat_observed's tables and statistic, and k_cat_permute's exceedance counts twice over -- from the code rows read
back and from the seed alone -- at the shapes where they can go wrong: one isolate, word and stage tails, the two
traits whose permuted tables tie exactly, every chunk boundary of the isolates, the largest matrix, empty classes,
traits of 0, 1 and 2 labelled isolates, one batch against two, counts that start above zero."""
import numpy as np
import pytest

import categorical_spec as cs

pytestmark = pytest.mark.gpu
SEED = 0x5EED0C47
ERR_SIZE = -3
CHUNK = 2432                                   # isolates of a chunk of k_cat_permute (kCatChunk)
TIE_VECTORS = {9: ([3, 3, 3], [(1, 1, 2), (2, 1, 1)]), 21: ([6, 3, 12], [(1, 2, 5), (3, 0, 5), (3, 2, 3)])}


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _gene_with_table(codes, a):
    """A 0/1 row that carries the first a_k isolates of class k."""
    gene, left = np.zeros(len(codes), dtype=np.uint8), list(a)
    for i, c in enumerate(codes):
        if c and left[c - 1] > 0:
            gene[i], left[c - 1] = 1, left[c - 1] - 1
    return gene


def _shape(name):
    """(genes [G, N] 0/1, codes [T, N], P, batches): the small shapes carry every kind of trait and gene."""
    N, P, batches = {"n1": (1, 1, 1), "tie9": (9, 500, 1), "tie21": (21, 500, 1), "n31": (31, 63, 1), "n32": (32, 64, 1),
                     "n33": (33, 65, 1), "n64": (64, 130, 2), "n65": (65, 130, 1),
                     "largest": (cs.MAX_ISOLATES, 10, 1)}.get(name, (0, 3, 1))
    if name.startswith("chunk"):               # at and one past a chunk boundary
        N = int(name[5:])
    rng = np.random.default_rng(sum(map(ord, name)))
    big = N > 1000
    traits = []
    if N in TIE_VECTORS:                       # the tie trait: balanced (3, 3, 3), or (6, 3, 12)
        traits.append(np.repeat(np.arange(1, 4), TIE_VECTORS[N][0]))
    k3 = rng.integers(0, 4, N)                 # K = 3 with missing isolates
    k8 = rng.integers(1, 9, N)                 # K = 8, no missing isolate
    traits += [k3, k8]
    if not big:
        k1 = (rng.random(N) < 0.8).astype(np.int64)                       # K = 1: untestable
        k2 = rng.integers(1, 3, N)
        gap = rng.choice([0, 1, 3], N)                                    # class 2 is empty among the valid isolates
        n0, n1, n2 = (np.zeros(N, dtype=np.int64) for _ in range(3))      # n = 0, 1, 2
        n1[N // 2] = 2
        n2[0], n2[N - 1] = 1, 2                                           # (n = 1 where N = 1)
        traits += [k1, k2, gap, n0, n1, n2]
    codes = np.stack(traits).astype(np.int64)
    G = 300 if big else 70                     # no multiple of the 64 genes of a block's step
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[1] = 0                               # m = 0
    genes[2] = 1                               # m = n
    genes[3] = 0
    genes[3, N - 1] = 1                        # one isolate, the last
    genes[4] = 1
    genes[4, 0] = 0                            # all but one isolate
    genes[5] = rng.random(N) < 0.9             # above half of the valid isolates
    t3 = 1 if N in TIE_VECTORS else 0
    genes[6] = codes[t3] == 0                  # carried only by isolates without a label (trait K = 3)
    genes[7] = codes[t3 + 1] == 1              # equal to a class of the K = 8 trait: X2 = n
    if N in TIE_VECTORS:
        for j, a in enumerate(TIE_VECTORS[N][1]):
            genes[8 + j] = _gene_with_table(codes[0], a)
    return genes, codes, P, batches


def _tables(genes, rows, K=8):
    """a[.., g, k] of 0/1 genes [G, N] against code rows [.., N] (ints): exact, in numpy (counts far below 2^24)."""
    onehot = (np.asarray(rows)[..., None] == np.arange(1, K + 1)).astype(np.float32)      # [.., N, K]
    parts = [np.einsum("gn,...nk->...gk", genes[g0:g0 + 8192].astype(np.float32), onehot, optimize=True)
             for g0 in range(0, len(genes), 8192)]
    return np.rint(np.concatenate(parts, axis=-2)).astype(np.int64)


def _r_exact(a_perm, a_obs, nk):
    """#{p : sum a_perm^2 L / n_k >= sum a_obs^2 L / n_k} per gene in integers (L / n_k from the restatement; Python
    integers where the sums could leave int64): a_perm [P, G, 8], a_obs [G, 8] -> [G]."""
    w = cs.weights([int(x) for x in nk])
    kind = np.int64 if max(w) < 1 << 31 else object        # a^2 < 2^28 and eight terms
    w = np.array(w, dtype=kind)
    s_perm = (a_perm.astype(kind) ** 2) @ w
    s_obs = (a_obs.astype(kind) ** 2) @ w
    return (s_perm >= s_obs[None]).sum(axis=0).astype(np.int64)


_CACHE = {}


def _case(eng, name):
    """Everything one shape needs, computed once: the device results and the restatement's rows."""
    import torch
    if name in _CACHE:
        return _CACHE[name]
    genes, codes, P, batches = _shape(name)
    T, N = codes.shape
    gm = eng.pack_dense(genes)
    plan = eng.categorical_plan(codes)
    obs = eng.categorical(gm, plan)
    res = {k: v.cpu().numpy() for k, v in obs.items()}
    rows = eng.categorical_rows(plan, 0, P, SEED).cpu().numpy()
    budget = (8 << 30) if batches == 1 else 2 * (2 * 64 * T * N)           # two stages of 64 permutations per batch
    assert -(-P // eng.categorical_batch(T, N, P, budget)) == batches
    r = eng.categorical_permute(gm, plan, obs["a"], P, SEED, budget_bytes=budget).cpu().numpy()
    # the same counts in one call on the rows read back, on top of counts that start at 5
    r5 = torch.full((T, len(genes)), 5, dtype=torch.int32, device=eng.device)
    eng.permute_categorical(gm, plan, obs["a"], torch.from_numpy(rows).to(eng.device), r5)
    spec_rows = np.array([[cs.perm_row(SEED, t, pi, codes[t].tolist()) for pi in range(P)] for t in range(T)])
    _CACHE[name] = dict(genes=genes, codes=codes, P=P, plan=plan, res=res, rows=rows, r=r, r5=r5.cpu().numpy(),
                        spec_rows=spec_rows)
    return _CACHE[name]


SMALL = ("n1", "tie9", "tie21", "n31", "n32", "n33", "n64", "n65")
BOUNDARIES = tuple("chunk%d" % (k * CHUNK + d) for k in range(1, cs.MAX_ISOLATES // CHUNK + 1) for d in (0, 1))
CASES = SMALL + BOUNDARIES + ("largest",)


def test_the_cases_cover_every_chunk_boundary():
    assert cs.MAX_ISOLATES // CHUNK == 6 and len(BOUNDARIES) == 12 and BOUNDARIES[-1] == "chunk14593"


@pytest.mark.parametrize("name", CASES)
def test_observed_tables_and_statistic(eng, name):
    c = _case(eng, name)
    genes, codes, res, plan = c["genes"], c["codes"], c["res"], c["plan"]
    T, N = codes.shape
    kinds = set()
    worst_p = worst_v = 0.0
    for t in range(T):
        row = codes[t].tolist()
        K = max(1, max(row))
        nk = cs.sizes(row, 8)
        assert plan.nk_host[t].tolist() == nk and int(plan.n[t]) == sum(nk)
        assert [int(x) for x in plan.weights[t]] == cs.weights(nk)
        a = _tables(genes, codes[t])
        for g in (0, 3, len(genes) - 1):
            assert a[g].tolist() == cs.table(genes[g].tolist(), row, 8)
        assert np.array_equal(res["a"][t], a) and np.array_equal(res["m"][t], a.sum(axis=1))      # bit for bit
        for g in range(len(genes)):
            ok, x2, df, p, v = cs.statistic(a[g, :K].tolist(), nk[:K])
            assert res["x2"][t, g] == x2, (t, g)                                                     # bit for bit
            kinds.add("testable" if ok else "untestable")
            if not ok:
                assert (res["p"][t, g], res["v"][t, g]) == (1.0, 0.0)
                continue
            assert abs(res["v"][t, g] - v) <= 2.0 ** -52 * v
            worst_v = max(worst_v, abs(res["v"][t, g] - v) / v if v > 0 else 0.0)
            if p > 1e-290:
                assert abs(res["p"][t, g] - p) <= 1e-10 * p, (t, g, res["p"][t, g], p)
                worst_p = max(worst_p, abs(res["p"][t, g] - p) / p)
    print("%s: worst relative error of p %.3g, of V %.3g" % (name, worst_p, worst_v))
    assert "untestable" in kinds and (N == 1 or "testable" in kinds)
    t = 2 if N in TIE_VECTORS else 1
    if 0 < genes[7].sum() < N:                 # the gene that equals a class of the K = 8 trait: X2 = n
        assert abs(res["x2"][t, 7] - N) <= 1e-12 * N and res["v"][t, 7] == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize("name", CASES)
def test_rows_are_the_shuffle_of_the_seed_and_keep_the_class_sizes(eng, name):
    c = _case(eng, name)
    assert np.array_equal(c["rows"], c["spec_rows"])
    want = np.sort(c["codes"], axis=1)
    assert np.array_equal(np.sort(c["rows"], axis=2), np.broadcast_to(want[:, None], c["rows"].shape))


@pytest.mark.parametrize("name", CASES)
def test_exceedance_counts_from_the_rows_and_from_the_seed(eng, name):
    c = _case(eng, name)
    genes, codes, P = c["genes"], c["codes"], c["P"]
    for t in range(codes.shape[0]):
        row = codes[t].tolist()
        nk = cs.sizes(row, 8)
        a_obs = _tables(genes, codes[t])
        from_rows = _r_exact(_tables(genes, c["rows"][t]), a_obs, nk)
        from_seed = _r_exact(_tables(genes, c["spec_rows"][t]), a_obs, nk)
        for g in (0, 5, 8, len(genes) - 1)[:4 if len(row) < 1000 else 2]:   # the numpy count is the restatement's
            assert from_seed[g] == cs.r_count(genes[g].tolist(), c["spec_rows"][t].tolist(), row, 8)
        assert np.array_equal(c["r"][t], from_rows), (name, t)
        assert np.array_equal(c["r"][t], from_seed), (name, t)
        assert np.array_equal(c["r5"][t], from_rows + 5), (name, t)
        for g in range(len(genes)):                                      # an untestable gene: r = P
            if not cs.testable(a_obs[g].tolist(), nk):
                assert c["r"][t, g] == P


@pytest.mark.parametrize("N", [33, CHUNK + 1])
def test_blocks_that_walk_several_gene_groups(eng, N):
    """More gene groups than a launch has ranges: a block walks several groups -- with one chunk of isolates on the
    rows it loaded once, with two on rows it loads again for every group."""
    rng = np.random.default_rng(N)
    G, T, P = 64 * 520 + 6, 2, 3
    genes = (rng.random((G, N)) < rng.uniform(0.0, 1.0, (G, 1))).astype(np.uint8)
    codes = np.stack([rng.integers(0, 4, N), rng.integers(1, 9, N)])
    gm = eng.pack_dense(genes)
    plan = eng.categorical_plan(codes)
    obs = eng.categorical(gm, plan)
    r = eng.categorical_permute(gm, plan, obs["a"], P, SEED).cpu().numpy()
    for t in range(T):
        rows = np.array([cs.perm_row(SEED, t, pi, codes[t].tolist()) for pi in range(P)])
        a_obs = _tables(genes, codes[t])
        assert np.array_equal(obs["a"][t].cpu().numpy(), a_obs)
        assert np.array_equal(r[t], _r_exact(_tables(genes, rows), a_obs, cs.sizes(codes[t].tolist(), 8))), t


@pytest.mark.parametrize("name", ["tie9", "tie21"])
def test_the_tie_traits_meet_exact_ties_that_an_fp64_sum_would_miss(eng, name):
    c = _case(eng, name)
    genes, codes = c["genes"], c["codes"]
    nk, vectors = TIE_VECTORS[codes.shape[1]]
    assert cs.sizes(codes[0].tolist(), 3) == nk
    missed = 0
    for j, a_obs in enumerate(vectors):
        g = 8 + j
        assert cs.table(genes[g].tolist(), codes[0].tolist(), 3) == list(a_obs)
        perm = _tables(genes[g:g + 1], c["spec_rows"][0], K=3)[:, 0].tolist()
        exact = sum(1 for a in perm if cs.exceeds(a, a_obs, nk))
        fp64 = sum(1 for a in perm if cs.s_fp64(a, nk) >= cs.s_fp64(a_obs, nk))
        ties = sum(1 for a in perm if a != list(a_obs) and cs.s_exact(a, nk) == cs.s_exact(a_obs, nk))
        assert c["r"][0, g] == exact and fp64 <= exact and ties > 0
        missed += exact - fp64                 # permutations that tie exactly and an fp64 comparison calls smaller
    assert missed > 0                          # at this seed: the case cannot pass vacuously


def test_sizes_past_the_limits_are_refused_with_nothing_written(eng):
    import torch
    G, T, N, P = 10, 1, 40, 5
    gm = eng.pack_dense(np.ones((G, N), dtype=np.uint8))
    plan = eng.categorical_plan(np.ones((T, N), dtype=np.int64))
    pat = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=eng.device)        # noqa: E731
    a, m, r = pat((T, G, 8), torch.int32), pat((T, G), torch.int32), pat((T, G), torch.int32)
    x2, p, v = (pat((T, G), torch.float64) for _ in range(3))
    rows = torch.zeros((T, P, N), dtype=torch.int16, device=eng.device)
    ptr = eng._ptr
    big = eng.ranksum_max_isolates() + 1
    assert eng.categorical_max_classes() == 8
    for K, n in ((9, N), (0, N), (3, big)):
        rc = eng.lib.scoary_categorical(eng.h, ptr(gm.tiled), ptr(plan.codes), ptr(plan.nk), G, T, n, K, ptr(a), ptr(m),
                                        ptr(x2), ptr(p), ptr(v), eng._stream())
        assert rc == ERR_SIZE, (K, n, rc)
    rc = eng.lib.scoary_permute_categorical(eng.h, ptr(gm.tiled), ptr(rows), ptr(a), ptr(plan.nk), ptr(plan.w), G, T,
                                            big, P, ptr(r), eng._stream())
    assert rc == ERR_SIZE
    rc = eng.lib.scoary_permute_categorical(eng.h, ptr(gm.tiled), ptr(rows), ptr(a), ptr(plan.nk), ptr(plan.w), G, T,
                                            N, 1 << 31, ptr(r), eng._stream())
    assert rc == ERR_SIZE
    torch.cuda.synchronize()
    for x in (a, m, r, x2, p, v):
        assert bool((x == 77).all())
    with pytest.raises(ValueError, match="a code is 0 .missing. or a class 1 .. 8"):
        eng.categorical_plan(np.full((1, 4), 9))


def test_a_row_with_codes_outside_the_classes_stays_inside_the_buffers(eng):
    """Codes that are none of the trait's (negative, past 8) are clamped: wrong numbers, the neighbours untouched."""
    import torch
    genes, codes, _P, _b = _shape("n33")
    gm = eng.pack_dense(genes)
    plan = eng.categorical_plan(codes[:1])
    obs = eng.categorical(gm, plan)
    rows = torch.tensor([-32768, 32767, 9, -1, 8] * 33, dtype=torch.int16, device=eng.device)[:2 * 33].reshape(1, 2, 33)
    guard = torch.full((3, len(genes)), 9, dtype=torch.int32, device=eng.device)
    eng.permute_categorical(gm, plan, obs["a"], rows.contiguous(), guard[1:2])
    torch.cuda.synchronize()
    got = guard.cpu().numpy()
    assert (got[0] == 9).all() and (got[2] == 9).all() and ((got[1] >= 9) & (got[1] <= 11)).all()
