"""The Westfall-Young kernels of the categorical traits (spec S22) on the GPU against the plain-Python restatement
(cat_wy_spec.py on top of categorical_spec.py and gcmh_spec.py): k_cat_wy_prepare's inv, ivm, s_obs and thr, and the
maxima and counts of k_cat_maxt and k_gcmh_maxt, bit for bit, through the raw entry points and through the engine -- at
the shapes where they can go wrong: one isolate, word and stage tails, ragged wavefronts and gene groups, one and two
chunks of isolates, blocks that walk several gene groups, three and seven class planes, empty classes, a trait of one
class, isolates without a label, strata of one and two isolates, rank-deficient forms, garbage behind the rows, a
sentinel behind every row of maxs, maxs that start above, at and below the result, and one batch against two."""
import numpy as np
import pytest

import cat_wy_spec as ws
import categorical_spec as cs
import gcmh_spec as gs

pytestmark = pytest.mark.gpu
SEED = 0x5EED22C4
ERR_ARG, ERR_SIZE = -1, -3
CHUNK = 2432                                   # isolates of a chunk of the kernels (kCatChunk)
SENTINEL = -7.25                               # behind every row of maxs: no maximum of s is negative
# name: (N, G, P, strata of the gcmh run)
SHAPES = {"n1": (1, 1, 1, 1), "n31": (31, 63, 63, 5), "n33": (33, 64, 64, 1), "chunk2432": (CHUNK, 65, 65, 4),
          "chunk2433": (CHUNK + 1, 129, 130, 2)}
CASES = tuple(SHAPES)


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
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _tables(genes, rows, K=8):
    """a[.., g, k] of 0/1 genes [G, N] against code rows [.., N] (ints): exact, in numpy (counts far below 2^24)."""
    onehot = (np.asarray(rows)[..., None] == np.arange(1, K + 1)).astype(np.float32)      # [.., N, K]
    parts = [np.einsum("gn,...nk->...gk", genes[g0:g0 + 8192].astype(np.float32), onehot, optimize=True)
             for g0 in range(0, len(genes), 8192)]
    return np.rint(np.concatenate(parts, axis=-2)).astype(np.int64)


def _shape(name):
    """(genes [G, N] 0/1, codes [T, N], strata [N]): T = 5 traits of different K -- three classes with missing
    isolates (three planes), eight classes (seven planes), an empty class in the middle, one class only (every gene
    untestable) and five classes of which the last lives in one stratum alone (a rank-deficient form)."""
    N, G, _P, S = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "n31":
        strata = np.repeat(np.arange(5), [12, 12, 4, 2, 1])              # strata of 2 and 1 isolates
    else:
        strata = rng.integers(0, S, N)
        strata[N - 1] = S - 1
    k3 = rng.integers(0, 4, N)
    k8 = rng.integers(1, 9, N)
    gap = rng.choice([0, 1, 3], N)
    one = (rng.random(N) < 0.8).astype(np.int64)
    only5 = rng.integers(1, 5, N)
    only5[(strata == 0) & (rng.random(N) < 0.4)] = 5                    # class 5 is confined to stratum 0
    codes = np.stack([k3, k8, gap, one, only5]).astype(np.int64)
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    if G > 8:
        genes[1] = 0                           # m = 0
        genes[2] = 1                           # m = n
        genes[3] = codes[0] == 0               # carried only by isolates without a label (first trait)
        genes[4] = codes[1] == 1               # equal to a class of the second trait: X2 = n, the largest there is
        genes[5, strata == 0] = 0              # absent from the stratum that holds class 5
    return genes, codes, strata


def _garbage_behind(eng, rows):
    """The rows [T, P, N] at the front of a buffer whose rest -- where a stage's pad permutations would be read --
    holds codes of every class."""
    import torch
    T, P, N = rows.shape
    buf = torch.randint(1, 9, ((T * P + 64) * N,), dtype=torch.int16, device=eng.device)
    buf[:T * P * N] = rows.reshape(-1)
    return buf[:T * P * N].view(T, P, N)


def _maxs_with_sentinels(eng, T, P):
    import torch
    maxs = torch.zeros((T, P + 3), dtype=torch.float64, device=eng.device)
    maxs[:, P:] = SENTINEL
    return maxs


_CACHE = {}


def _chi2(eng, name):
    """The chi-square run of a shape, computed once: the device results through the raw entry points on the rows read
    back, through the engine from the seed, and the restatement."""
    import torch
    if ("chi2", name) in _CACHE:
        return _CACHE[("chi2", name)]
    genes, codes, _strata = _shape(name)
    N, G, P, _S = SHAPES[name]
    T = codes.shape[0]
    gm = eng.pack_dense(genes)
    plan = eng.categorical_plan(codes)
    obs = eng.categorical(gm, plan)
    ptr = eng._ptr
    # prepare with K = 8: the classes from a trait's K on are empty ones
    inv = torch.full((T, 8), 77.0, dtype=torch.float64, device=eng.device)
    ivm, sobs, thr = (torch.full((T, G), 77.0, dtype=torch.float64, device=eng.device) for _ in range(3))
    rc = eng.lib.scoary_cat_wy_prepare(eng.h, ptr(obs["a"]), ptr(plan.nk), G, T, 8, ptr(inv), ptr(ivm), ptr(sobs),
                                       ptr(thr), eng._stream())
    assert rc == 0
    einv, eivm, esobs, ethr = eng.categorical_wy_prepare(plan, obs["a"])      # (with the plan's K)
    rows = eng.categorical_rows(plan, 0, P, SEED)
    padded = _garbage_behind(eng, rows)
    r5 = torch.full((T, G), 5, dtype=torch.int32, device=eng.device)
    p5 = torch.full((T, G), 5, dtype=torch.int32, device=eng.device)
    maxs = _maxs_with_sentinels(eng, T, P)
    rc = eng.lib.scoary_permute_cat_wy(eng.h, ptr(gm.tiled), ptr(padded), ptr(obs["a"]), ptr(plan.nk), ptr(plan.w),
                                       ptr(inv), ptr(ivm), G, T, N, P, ptr(r5), ptr(maxs), P + 3, eng._stream())
    assert rc == 0
    eng.permute_categorical(gm, plan, obs["a"], padded, p5)                   # k_cat_permute on the same rows, from 5
    # the engine, from the seed, in two batches where P allows it
    budget = (8 << 30) if P <= 128 else 2 * (2 * 64 * T * N)
    r, r_fwer, emaxs = eng.categorical_westfall_young(gm, plan, obs, P, SEED, budget_bytes=budget)
    spec = []
    a_obs, a_perm = _tables(genes, codes), _tables(genes, rows.cpu().numpy())          # [T, G, 8], [T, P, G, 8]
    for t in range(T):
        nk = cs.sizes(codes[t].tolist(), 8)
        ivm_t = np.array([ws.ivm_of(a.tolist(), nk) for a in a_obs[t]])
        s_obs = ws.stats(a_obs[t], nk, ivm_t)
        cells = ws.stats(a_perm[t], nk, ivm_t)                                           # [P, G]
        spec.append(dict(nk=nk, inv=np.array(ws.inv_of(nk)), ivm=ivm_t, s_obs=s_obs, thr=ws.thr_of(s_obs),
                         cells=cells, maxs=ws.maxs(cells)))
    _CACHE[("chi2", name)] = dict(
        genes=genes, codes=codes, gm=gm, plan=plan, obs=obs, rows=rows, padded=padded, a_obs=a_obs, a_perm=a_perm,
        spec=spec, dev={k: v.cpu().numpy() for k, v in dict(inv=inv, ivm=ivm, s_obs=sobs, thr=thr, einv=einv,
                                                             eivm=eivm, es_obs=esobs, ethr=ethr, r5=r5, p5=p5,
                                                             maxs=maxs, r=r, r_fwer=r_fwer, emaxs=emaxs).items()},
        tensors=dict(inv=inv, ivm=ivm, thr=thr))
    return _CACHE[("chi2", name)]


def test_the_shapes_reach_every_branch():
    assert sorted(s[0] for s in SHAPES.values()) == [1, 31, 33, CHUNK, CHUNK + 1]
    assert sorted(s[1] for s in SHAPES.values()) == [1, 63, 64, 65, 129]
    assert sorted(s[2] for s in SHAPES.values()) == [1, 63, 64, 65, 130]
    _genes, codes, strata = _shape("n31")
    assert sorted(np.bincount(strata))[:2] == [1, 2]
    assert [int(row.max()) for row in codes] == [3, 8, 3, 1, 5] and 2 not in codes[2]
    assert set(strata[codes[4] == 5]) == {0}


@pytest.mark.parametrize("name", CASES)
def test_prepare_is_the_restatement_bit_for_bit(eng, name):
    c = _chi2(eng, name)
    kinds = set()
    for t, sp in enumerate(c["spec"]):
        for g in sorted({0, len(c["genes"]) - 1}):                       # the array route is the scalar restatement's
            a = c["a_obs"][t, g].tolist()
            assert sp["ivm"][g] == ws.ivm_of(a, sp["nk"]) and sp["s_obs"][g] == ws.stat(a, sp["nk"], sp["ivm"][g])
        for key in ("inv", "ivm", "s_obs", "thr"):
            assert np.array_equal(_bits(c["dev"][key][t]), _bits(sp[key])), (name, t, key)
            assert np.array_equal(_bits(c["dev"]["e" + key][t]), _bits(sp[key])), (name, t, key)       # the engine's
        kinds |= {"testable" if x > 0 else "untestable" for x in sp["ivm"]}
        untestable = sp["ivm"] == 0
        assert not c["dev"]["s_obs"][t][untestable].any() and not c["dev"]["thr"][t][untestable].any()
        ok = ~untestable
        x2 = c["obs"]["x2"][t].cpu().numpy()
        assert np.allclose(c["dev"]["s_obs"][t][ok], x2[ok], rtol=1e-14, atol=0)          # S20's X2, to rounding
    assert "untestable" in kinds and (SHAPES[name][0] == 1 or "testable" in kinds)


@pytest.mark.parametrize("name", CASES)
def test_chi2_maxima_and_counts_are_the_restatement_bit_for_bit(eng, name):
    c = _chi2(eng, name)
    N, G, P, _S = SHAPES[name]
    dev = c["dev"]
    assert (dev["maxs"][:, P:] == SENTINEL).all()                        # nothing behind a row's P columns
    assert np.array_equal(dev["r5"], dev["p5"])                          # d_r is scoary_permute_categorical's, from 5
    for t, sp in enumerate(c["spec"]):
        assert np.array_equal(_bits(dev["maxs"][t, :P]), _bits(sp["maxs"])), (name, t)
        assert np.array_equal(_bits(dev["emaxs"][t]), _bits(sp["maxs"])), (name, t)      # the engine, from the seed
        want = ws.r_fwer(sp["maxs"], sp["thr"])
        assert np.array_equal(dev["r_fwer"][t], want), (name, t)
        assert np.array_equal(dev["r"][t], dev["r5"][t] - 5), (name, t)
        assert (dev["r_fwer"][t] >= dev["r"][t]).all()
        assert (dev["r_fwer"][t][sp["s_obs"] == 0] == P).all()
        order = np.argsort(sp["s_obs"], kind="stable")
        assert (np.diff(dev["r_fwer"][t][order]) <= 0).all()             # does not increase with s_obs
        # the count itself, in integers, from the tables the restatement made
        w = np.array(cs.weights(sp["nk"]), dtype=object)
        exact = ((c["a_perm"][t].astype(object) ** 2) @ w >= ((c["a_obs"][t].astype(object) ** 2) @ w)[None]).sum(axis=0)
        assert np.array_equal(dev["r"][t], exact.astype(np.int64)), (name, t)
    one = 3                                                              # the trait of one class: maxs = 0, r_fwer = P
    assert not dev["maxs"][one, :P].any() and (dev["r_fwer"][one] == P).all()
    if N > 1:
        assert (dev["maxs"][1, :P] > 0).all()


def test_the_rows_of_the_small_shapes_are_the_shuffle_of_the_seed(eng):
    for name in ("n1", "n31", "n33"):
        c = _chi2(eng, name)
        codes, P = c["codes"], SHAPES[name][2]
        spec_rows = np.array([[cs.perm_row(SEED, t, pi, codes[t].tolist()) for pi in range(P)]
                              for t in range(codes.shape[0])])
        assert np.array_equal(c["rows"].cpu().numpy(), spec_rows)


def test_a_maxs_that_starts_above_at_and_below_the_result(eng):
    import torch
    c = _chi2(eng, "n33")
    N, G, P, _S = SHAPES["n33"]
    T = c["codes"].shape[0]
    want = np.stack([sp["maxs"] for sp in c["spec"]])
    start = want.copy()
    start[:, 0] = want[:, 0] + 1.0                                       # above
    start[:, 2] = np.nextafter(want[:, 2], -1.0)                         # one ulp below (0 stays 0: the one-class trait)
    start[:, 2] = np.maximum(start[:, 2], 0.0)
    start[:, 3:] = 0.0
    maxs = torch.from_numpy(np.concatenate([start, np.full((T, 3), SENTINEL)], axis=1)).to(eng.device)
    r = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    t_ = c["tensors"]
    eng.permute_categorical(c["gm"], c["plan"], c["obs"]["a"], c["padded"], r, maxt=(t_["inv"], t_["ivm"], maxs))
    got = maxs.cpu().numpy()
    assert np.array_equal(_bits(got[:, :P]), _bits(np.maximum(start, want))) and (got[:, P:] == SENTINEL).all()
    assert (got[:, 0] > want[:, 0]).all() and np.array_equal(_bits(got[:, 1:P]), _bits(want[:, 1:]))
    assert (start[1, 2] < want[1, 2])                                    # (the ulp below was one)


def test_two_batches_of_64_against_one_of_128_and_a_repeat(eng):
    genes, codes, strata = _shape("n33")
    T, N, P = codes.shape[0], codes.shape[1], 128
    gm = eng.pack_dense(genes)
    plan = eng.categorical_plan(codes)
    obs = eng.categorical(gm, plan)
    one = eng.categorical_westfall_young(gm, plan, obs, P, SEED)
    assert eng.categorical_batch(T, N, P, 2 * 64 * T * N) == 64
    two = eng.categorical_westfall_young(gm, plan, obs, P, SEED, budget_bytes=2 * 64 * T * N)
    again = eng.categorical_westfall_young(gm, plan, obs, P, SEED)
    for x, y, z in zip(one, two, again):                                 # (r, r_fwer, maxs): int32 is exact in a double
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(z.cpu().numpy()))
    gplan = eng.gcmh_plan(codes, strata)
    gobs = eng.gcmh(gm, gplan)
    one = eng.gcmh_westfall_young(gm, gplan, gobs, P, SEED)
    two = eng.gcmh_westfall_young(gm, gplan, gobs, P, SEED, budget_bytes=2 * 64 * T * N)
    again = eng.gcmh_westfall_young(gm, gplan, gobs, P, SEED)
    for x, y, z in zip(one, two, again):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(z.cpu().numpy()))


# ---- the generalized CMH maximum ----
def _gspec(genes, row, strata, S):
    """The restatement of one trait over all genes: dict(a, form, df, q, thr)."""
    row = np.asarray(row)
    nsk = gs.margins(row.tolist(), strata.tolist(), S)
    member = ((strata[:, None] == np.arange(S)) & (row[:, None] != 0)).astype(np.float32)          # [N, S]
    ms = np.rint(genes.astype(np.float32) @ member).astype(np.int64)
    a = _tables(genes, row)
    E, V = gs.moments_many(ms, nsk)
    form, df = gs.factor_many(E, V, max(gs.klast(nsk) - 1, 0))
    q = gs.q_many(a, form)
    return dict(a=a, form=form, df=df, q=q, thr=q * gs.ONE_MINUS_TAU)


def _gcmh(eng, name):
    import torch
    if ("gcmh", name) in _CACHE:
        return _CACHE[("gcmh", name)]
    genes, codes, strata = _shape(name)
    N, G, P, S = SHAPES[name]
    T = codes.shape[0]
    gm = eng.pack_dense(genes)
    plan = eng.gcmh_plan(codes, strata)
    assert plan.S == S
    obs = eng.gcmh(gm, plan)
    rows = eng.gcmh_rows(plan, 0, P, SEED)
    padded = _garbage_behind(eng, rows)
    ptr = eng._ptr
    r5 = torch.full((T, G), 5, dtype=torch.int32, device=eng.device)
    p5 = torch.full((T, G), 5, dtype=torch.int32, device=eng.device)
    maxs = _maxs_with_sentinels(eng, T, P)
    rc = eng.lib.scoary_permute_gcmh_wy(eng.h, ptr(gm.tiled), ptr(padded), ptr(obs["form"]), ptr(obs["thr"]),
                                        ptr(plan.nk), G, T, N, P, ptr(r5), ptr(maxs), P + 3, eng._stream())
    assert rc == 0
    eng.permute_gcmh(gm, plan, obs, padded, p5)                               # k_gcmh_permute on the same rows, from 5
    budget = (8 << 30) if P <= 128 else 2 * (2 * 64 * T * N)
    r, r_fwer, emaxs = eng.gcmh_westfall_young(gm, plan, obs, P, SEED, budget_bytes=budget)
    spec = []
    for t in range(T):
        sp = _gspec(genes, codes[t], strata, S)
        sp["cells"] = gs.q_many(_tables(genes, rows[t].cpu().numpy()), sp["form"])       # [P, G]
        sp["maxs"] = ws.maxs(sp["cells"])
        spec.append(sp)
    _CACHE[("gcmh", name)] = dict(genes=genes, codes=codes, strata=strata, spec=spec, obs=obs,
                                  dev={k: v.cpu().numpy() for k, v in dict(r5=r5, p5=p5, maxs=maxs, r=r, r_fwer=r_fwer,
                                                                           emaxs=emaxs, q=obs["q"], thr=obs["thr"],
                                                                           df=obs["df"]).items()})
    return _CACHE[("gcmh", name)]


@pytest.mark.parametrize("name", CASES)
def test_gcmh_maxima_and_counts_are_the_restatement_bit_for_bit(eng, name):
    c = _gcmh(eng, name)
    N, G, P, S = SHAPES[name]
    dev = c["dev"]
    assert (dev["maxs"][:, P:] == SENTINEL).all()
    assert np.array_equal(dev["r5"], dev["p5"])                          # d_r is scoary_permute_gcmh's, from 5
    dfs = set()
    for t, sp in enumerate(c["spec"]):
        assert np.array_equal(_bits(dev["q"][t]), _bits(sp["q"]))
        assert np.array_equal(_bits(dev["thr"][t]), _bits(sp["thr"]))
        assert np.array_equal(_bits(dev["maxs"][t, :P]), _bits(sp["maxs"])), (name, t)
        assert np.array_equal(_bits(dev["emaxs"][t]), _bits(sp["maxs"])), (name, t)
        assert np.array_equal(dev["r_fwer"][t], ws.r_fwer(sp["maxs"], sp["thr"])), (name, t)
        assert np.array_equal(dev["r"][t], (sp["cells"] >= sp["thr"][None]).sum(axis=0)), (name, t)
        assert np.array_equal(dev["r"][t], dev["r5"][t] - 5)
        assert (dev["r_fwer"][t] >= dev["r"][t]).all()
        assert (dev["r_fwer"][t][sp["df"] == 0] == P).all()
        order = np.argsort(sp["thr"], kind="stable")
        assert (np.diff(dev["r_fwer"][t][order]) <= 0).all()
        dfs |= set(sp["df"].tolist())
    assert not dev["maxs"][3, :P].any() and (dev["r_fwer"][3] == P).all()    # the trait of one class
    if name == "n31":
        # class 5 lives in stratum 0 alone: the gene that is absent from it sees four classes, the others five
        df = c["spec"][4]["df"]
        assert df[5] == 3 and df.max() == 4 and 0 in dfs
    if name == "n33":
        # one stratum: Q is X2 (n - 1) / n, so the maximum is the restatement's of Q and not the chi-square one's
        assert S == 1
        chi = _chi2(eng, name)
        for t in (0, 1):
            n = sum(chi["spec"][t]["nk"])
            assert np.allclose(dev["maxs"][t, :P], chi["spec"][t]["maxs"] * (n - 1) / n, rtol=1e-12, atol=0)
            assert (dev["maxs"][t, :P] != chi["spec"][t]["maxs"]).all()


def test_one_gene_meets_its_own_count(eng):
    """G = 1: r_fwer = r for gcmh by itself, and for the chi-square test where no permuted table lies inside the band
    (checked on the inputs in the rationals)."""
    rng = np.random.default_rng(77)
    N, P = 40, 200
    gene = (rng.random((1, N)) < 0.4).astype(np.uint8)
    codes = np.stack([rng.integers(0, 4, N), rng.integers(1, 6, N)])
    strata = rng.integers(0, 3, N)
    strata[0] = 2
    gm = eng.pack_dense(gene)
    plan = eng.categorical_plan(codes)
    obs = eng.categorical(gm, plan)
    r, r_fwer, _maxs = eng.categorical_westfall_young(gm, plan, obs, P, SEED)
    rows = eng.categorical_rows(plan, 0, P, SEED).cpu().numpy()
    for t in range(2):
        nk = cs.sizes(codes[t].tolist(), 8)
        a_obs = cs.table(gene[0].tolist(), codes[t].tolist(), 8)
        assert cs.testable(a_obs, nk)
        assert not any(ws.inside_band(cs.table(gene[0].tolist(), row.tolist(), 8), a_obs, nk) for row in rows[t])
    assert np.array_equal(r.cpu().numpy(), r_fwer.cpu().numpy()) and 0 < int(r[0, 0]) < P
    gplan = eng.gcmh_plan(codes, strata)
    gobs = eng.gcmh(gm, gplan)
    r, r_fwer, _maxs = eng.gcmh_westfall_young(gm, gplan, gobs, P, SEED)
    assert np.array_equal(r.cpu().numpy(), r_fwer.cpu().numpy()) and 0 < int(r[0, 0]) < P


@pytest.mark.parametrize("N", [33, CHUNK + 1])
def test_blocks_that_walk_several_gene_groups(eng, N):
    """More gene groups than a launch has ranges: a block's running maximum lives across several groups -- with one
    chunk of isolates on the rows it loaded once, with two on rows it loads again for every group."""
    rng = np.random.default_rng(N)
    G, T, P, S = 64 * 520 + 6, 2, 3, 3
    genes = (rng.random((G, N)) < rng.uniform(0.0, 1.0, (G, 1))).astype(np.uint8)
    codes = np.stack([rng.integers(0, 4, N), rng.integers(1, 9, N)])
    strata = rng.integers(0, S, N)
    strata[0] = S - 1
    gm = eng.pack_dense(genes)
    plan = eng.categorical_plan(codes)
    obs = eng.categorical(gm, plan)
    r, r_fwer, maxs = (x.cpu().numpy() for x in eng.categorical_westfall_young(gm, plan, obs, P, SEED))
    plain = eng.categorical_permute(gm, plan, obs["a"], P, SEED).cpu().numpy()
    rows = eng.categorical_rows(plan, 0, P, SEED).cpu().numpy()
    a_obs, a_perm = _tables(genes, codes), _tables(genes, rows)
    assert np.array_equal(r, plain)
    for t in range(T):
        nk = cs.sizes(codes[t].tolist(), 8)
        ivm = np.array([ws.ivm_of(a.tolist(), nk) for a in a_obs[t]])
        cells = ws.stats(a_perm[t], nk, ivm)
        assert np.array_equal(_bits(maxs[t]), _bits(ws.maxs(cells))), t
        assert np.array_equal(r_fwer[t], ws.r_fwer(ws.maxs(cells), ws.thr_of(ws.stats(a_obs[t], nk, ivm)))), t
    gplan = eng.gcmh_plan(codes, strata)
    gobs = eng.gcmh(gm, gplan)
    r, r_fwer, maxs = (x.cpu().numpy() for x in eng.gcmh_westfall_young(gm, gplan, gobs, P, SEED))
    assert np.array_equal(r, eng.gcmh_permute(gm, gplan, gobs, P, SEED).cpu().numpy())
    grows = eng.gcmh_rows(gplan, 0, P, SEED).cpu().numpy()
    for t in range(T):
        sp = _gspec(genes, codes[t], strata, S)
        assert np.array_equal(_bits(gobs["thr"][t].cpu().numpy()), _bits(sp["thr"]))
        cells = gs.q_many(_tables(genes, grows[t]), sp["form"])
        assert np.array_equal(_bits(maxs[t]), _bits(ws.maxs(cells))), t
        assert np.array_equal(r_fwer[t], ws.r_fwer(ws.maxs(cells), sp["thr"])), t


def test_sizes_past_the_limits_and_a_short_stride_are_refused_with_nothing_written(eng):
    import torch
    G, T, N, P, S = 10, 1, 40, 5, 2
    gm = eng.pack_dense(np.ones((G, N), dtype=np.uint8))
    codes = (np.arange(N) % 3 + 1).reshape(1, N)
    plan = eng.categorical_plan(codes)
    gplan = eng.gcmh_plan(codes, np.arange(N) % S)
    obs, gobs = eng.categorical(gm, plan), eng.gcmh(gm, gplan)
    pat = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=eng.device)        # noqa: E731
    inv, ivm, sobs, thr = pat((T, 8), torch.float64), *(pat((T, G), torch.float64) for _ in range(3))
    r, maxs = pat((T, G), torch.int32), pat((T, P + 3), torch.float64)
    rows = torch.zeros((T, P, N), dtype=torch.int16, device=eng.device)
    ptr = eng._ptr
    big = eng.ranksum_max_isolates() + 1

    def prepare(g, t, K):
        return eng.lib.scoary_cat_wy_prepare(eng.h, ptr(obs["a"]), ptr(plan.nk), g, t, K, ptr(inv), ptr(ivm), ptr(sobs),
                                             ptr(thr), eng._stream())

    def chi2(g, t, n, pp, stride):
        return eng.lib.scoary_permute_cat_wy(eng.h, ptr(gm.tiled), ptr(rows), ptr(obs["a"]), ptr(plan.nk), ptr(plan.w),
                                             ptr(inv), ptr(ivm), g, t, n, pp, ptr(r), ptr(maxs), stride, eng._stream())

    def gcmh(g, t, n, pp, stride):
        return eng.lib.scoary_permute_gcmh_wy(eng.h, ptr(gm.tiled), ptr(rows), ptr(gobs["form"]), ptr(gobs["thr"]),
                                              ptr(gplan.nk), g, t, n, pp, ptr(r), ptr(maxs), stride, eng._stream())
    for g, t, K in ((G, T, 9), (G, T, 0), (G, 65536, 3), (1 << 31, T, 3)):
        assert prepare(g, t, K) == ERR_SIZE, (g, t, K)
    assert prepare(0, T, 3) == ERR_ARG
    for call in (chi2, gcmh):
        for g, t, n, pp in ((G, T, big, P), (G, T, N, 1 << 31), (G, 65536, N, P), (1 << 31, T, N, P)):
            assert call(g, t, n, pp, max(pp, P) + 3) == ERR_SIZE, (call.__name__, g, t, n, pp)
        assert call(G, T, N, P, P - 1) == ERR_ARG                       # maxs_stride < P
        assert call(G, T, N, 0, P) == ERR_ARG
    torch.cuda.synchronize()
    for x in (inv, ivm, sobs, thr, r, maxs):
        assert bool((x == 77).all())
    assert chi2(G, T, N, P, P) == 0 and gcmh(G, T, N, P, P) == 0        # (the arguments were sound otherwise)
    with pytest.raises(ValueError, match="maxs is float64"):
        eng.permute_categorical(gm, plan, obs["a"], rows, r, maxt=(inv, ivm, maxs[:, :P - 1]))
    with pytest.raises(ValueError, match="maxs is float64"):
        eng.permute_gcmh(gm, gplan, gobs, rows, r, maxt=maxs[:, :P - 1].to(torch.float32))


def test_the_lds_opt_in_is_taken_once_per_kernel_on_a_fresh_engine():
    """The four hot kernels on an engine of their own, each first at N = 1152 (36 plane words, 64 512 B of LDS: no
    opt-in), then at N = 1153 (40 words, 71 680 B: the kernel's first launch that needs the opt-in), then at N = 1153
    again (the handle's bit is set): counts and maxima are the restatement's, bit for bit, every time."""
    import torch
    from scoary_amd.engine import AssociationEngine
    G, T, P, K, S = 70, 1, 65, 5, 3
    fresh = AssociationEngine(0)
    try:
        want = {}
        for N in (1152, 1153, 1153):
            rng = np.random.default_rng(N)
            genes = (rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))).astype(np.uint8)
            codes = rng.integers(0, K + 1, (T, N))
            strata = rng.integers(0, S, N)
            strata[0] = S - 1
            gm = fresh.pack_dense(genes)
            plan, gplan = fresh.categorical_plan(codes), fresh.gcmh_plan(codes, strata)
            obs, gobs = fresh.categorical(gm, plan), fresh.gcmh(gm, gplan)
            inv, ivm, _sobs, _thr = fresh.categorical_wy_prepare(plan, obs["a"])
            rows, grows = fresh.categorical_rows(plan, 0, P, SEED), fresh.gcmh_rows(gplan, 0, P, SEED)
            zeros = lambda: torch.zeros((T, G), dtype=torch.int32, device=fresh.device)            # noqa: E731
            maxs, gmaxs = _maxs_with_sentinels(fresh, T, P), _maxs_with_sentinels(fresh, T, P)
            got = dict(r=fresh.permute_categorical(gm, plan, obs["a"], rows, zeros()),
                       r_maxt=fresh.permute_categorical(gm, plan, obs["a"], rows, zeros(), maxt=(inv, ivm, maxs)),
                       g=fresh.permute_gcmh(gm, gplan, gobs, grows, zeros()),
                       g_maxt=fresh.permute_gcmh(gm, gplan, gobs, grows, zeros(), maxt=gmaxs), maxs=maxs, gmaxs=gmaxs)
            got = {k: v.cpu().numpy() for k, v in got.items()}
            if N not in want:                                            # (the third round repeats the second's inputs)
                nk = cs.sizes(codes[0].tolist(), 8)
                a_obs, a_perm = _tables(genes, codes)[0], _tables(genes, rows.cpu().numpy())[0]
                ivm_t = np.array([ws.ivm_of(a.tolist(), nk) for a in a_obs])
                w = np.array(cs.weights(nk), dtype=object)
                exact = ((a_perm.astype(object) ** 2) @ w >= ((a_obs.astype(object) ** 2) @ w)[None]).sum(axis=0)
                sp = _gspec(genes, codes[0], strata, S)
                cells = gs.q_many(_tables(genes, grows[0].cpu().numpy()), sp["form"])
                want[N] = dict(r=exact.astype(np.int64), maxs=ws.maxs(ws.stats(a_perm, nk, ivm_t)),
                               g=(cells >= sp["thr"][None]).sum(axis=0), gmaxs=ws.maxs(cells))
                assert 0 < want[N]["r"].sum() < G * P and 0 < want[N]["g"].sum() < G * P and want[N]["maxs"].min() > 0
            for plain, fused, col in (("r", "r_maxt", "maxs"), ("g", "g_maxt", "gmaxs")):
                assert np.array_equal(got[plain][0], want[N][plain]), (N, plain)
                assert np.array_equal(got[fused][0], want[N][plain]), (N, fused)
                assert np.array_equal(_bits(got[col][0, :P]), _bits(want[N][col])), (N, col)
                assert (got[col][:, P:] == SENTINEL).all()
    finally:
        fresh.close()
