"""Westfall-Young family-wise p of the CMH statistic (spec S11): the tables of scoary_cmh_minp_plan / _fill, the
observed values, and minu / r_cmh_fwer / r_cmh_fwer_sd of the unchanged Westfall-Young passes over them -- every
comparison exact, against the plain-Python restatement (tests/cmh_wy_spec.py over cmh_spec.py) on label rows read
back from the S9 generator."""
import numpy as np
import pytest

import cmh_cases as C
import cmh_spec as S10
import cmh_wy_spec as S11
from cmh_cases import Case

pytestmark = pytest.mark.gpu
SEED = 20261019


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


# ---- the shapes -------------------------------------------------------------------------------------------------
def small_case():
    """N = 70, S = 4, G = 300 (off the 256-gene block), T = 5 (off the 4-trait block), missing values: stratum 1 has
    no member, stratum 2 one, and the members of stratum 3 are all invalid for trait 1."""
    N, G, T, S = 70, 300, 5, 4
    genes, traits, rng = C.random_genes_traits(G, N, T, S)
    strata = np.where(rng.random(N) < 0.6, 0, 3)
    strata[17] = 2
    traits[1, strata == 3] = 2
    traits[3, rng.random(N) < 0.1] = 2
    assert (strata == 1).sum() == 0 and (strata == 2).sum() == 1 and (traits[1] != 2).any()
    return genes, traits, strata, S


def wide_case():
    """N = 20 479 (rows of 160 quads: the chunked kernels), S = 3, G = 70, T = 2."""
    N, G, T, S = 20479, 70, 2, 3
    genes, traits, rng = C.random_genes_traits(G, N, T, S, dense_genes=True)
    return genes, traits, rng.integers(0, S, N), S


_CACHE = {}


def case_and_spec(eng, name):
    """(Case, spec) of a shape, built once per module: spec = dict of lo, off, tab, A, u_obs from cmh_wy_spec, and
    the per-stratum counts."""
    if name not in _CACHE:
        genes, traits, strata, S = {"small": small_case, "wide": wide_case}[name]()
        c = Case(eng, genes, traits, strata, S=S)
        a, m, k, n = c.recount()
        lo, off, tab, A = S11.csr(a, m, k, n)
        spec = {"lo": lo, "off": off, "tab": tab, "A": A, "u_obs": S11.observed(lo, off, tab, A),
                "amkn": (a, m, k, n)}
        for v in (lo, off, tab, A, spec["u_obs"]):
            v.setflags(write=False)
        _CACHE[name] = (c, spec)
    return _CACHE[name]


def device_tables(eng, c):
    """(cmh()'s result, the MinpTables built from it)."""
    res = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    tabs = eng.cmh_tables(c.gm, c.mkv, c.sp, res)
    return res, tabs


# ---- 1. tables --------------------------------------------------------------------------------------------------
def test_tables_equal_the_spec_bit_for_bit(eng):
    c, spec = case_and_spec(eng, "small")
    assert (c.G % 256, c.T % 4) != (0, 0) and (c.traits == 2).any()
    before = {k: v.cpu().numpy().copy() for k, v in eng.cmh(c.gm, c.trv, c.mkv, c.sp).items()}
    res, tabs = device_tables(eng, c)
    assert tabs.entries == len(spec["tab"]) == int(spec["off"][-1])
    assert np.array_equal(tabs.lo.cpu().numpy(), spec["lo"])
    assert np.array_equal(tabs.off.cpu().numpy(), spec["off"])
    assert np.array_equal(tabs.tab.cpu().numpy(), spec["tab"])
    sizes = np.diff(spec["off"])
    assert sizes.min() == 1 and sizes.max() > 8 and ((spec["tab"] > 0) & (spec["tab"] <= 1)).all()
    # scoary_cmh's outputs: the same before the plan call, after it and after the fill
    for key, v in before.items():
        assert np.array_equal(res[key].cpu().numpy(), v, equal_nan=True), key
    again = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    for key, v in before.items():
        assert np.array_equal(again[key].cpu().numpy(), v, equal_nan=True), key
    # the observed value is the gene's own entry, and 1 / (1 + stat) of scoary_cmh's stat wherever E2 is not snapped
    u_obs = eng.cmh_observed(tabs, res["a"]).cpu().numpy()
    assert np.array_equal(u_obs, spec["u_obs"])
    stat, e2 = before["stat"], before["e2"]
    dead = before["var"] == 0
    assert dead.any() and np.array_equal(np.isnan(stat), dead) and (u_obs[dead] == 1.0).all()
    snapped = np.array([[S11.snap(x) != x for x in row] for row in e2])
    keep = ~dead & ~snapped
    assert keep.sum() > c.T * c.G // 2
    assert np.array_equal(u_obs[keep], 1.0 / (1.0 + stat[keep]))
    # the support lies inside Fisher's
    counts = eng.counts(c.gm, c.trv, c.mkv)[0]
    fisher = eng.minp_tables(counts)
    flo, fsize = fisher.lo.cpu().numpy(), np.diff(fisher.off.cpu().numpy()).reshape(c.T, c.G)
    assert (spec["lo"] >= flo).all() and (spec["lo"] + sizes.reshape(c.T, c.G) <= flo + fsize).all()


# ---- 2. limits --------------------------------------------------------------------------------------------------
def test_tables_with_1024_random_strata(eng):
    N, S, G, T = 2100, 1024, 130, 1
    genes, traits, rng = C.random_genes_traits(G, N, T, S)
    c = Case(eng, genes, traits, rng.integers(0, S, N), S=S)
    lo, off, tab, _A = S11.csr(*c.recount())
    _res, tabs = device_tables(eng, c)
    assert np.array_equal(tabs.lo.cpu().numpy(), lo) and np.array_equal(tabs.off.cpu().numpy(), off)
    assert np.array_equal(tabs.tab.cpu().numpy(), tab)
    assert np.diff(off).max() > 100


def test_tables_at_the_most_isolates(eng):
    c, spec = case_and_spec(eng, "wide")
    assert c.N == int(eng.lib.scoary_perm_strata_max_isolates())
    _res, tabs = device_tables(eng, c)
    assert np.array_equal(tabs.lo.cpu().numpy(), spec["lo"]) and np.array_equal(tabs.off.cpu().numpy(), spec["off"])
    assert np.array_equal(tabs.tab.cpu().numpy(), spec["tab"])
    assert np.diff(spec["off"]).max() > 2000


def test_a_table_past_2_pow_24_entries(eng):
    """More than 2^24 + 2^20 entries in one build (about 200 MB): lo and off against numpy's integer sums for every
    gene, 2000 seeded entries and the first and last entry of the first and last gene against the spec."""
    N, S, G = 20479, 2, 5000
    rng = np.random.default_rng(5000)
    genes = rng.integers(0, 2, (G, N), dtype=np.uint8)
    trait = (rng.random(N) < 0.25).astype(np.uint8)[None]
    strata = (np.arange(N) >= 9000).astype(np.int64)
    c = Case(eng, genes, trait, strata, S=S)
    onehot = np.stack([strata == s for s in range(S)], axis=1).astype(np.float32)
    m = np.rint(genes.astype(np.float32) @ onehot).astype(np.int64)                       # [G, S]
    a = np.rint((genes & trait).astype(np.float32) @ onehot).astype(np.int64)
    k, n = np.bincount(strata[trait[0] == 1], minlength=S), np.bincount(strata, minlength=S)
    lo = np.maximum(0, k[None] + m - n[None]).sum(1)
    hi = np.minimum(k[None], m).sum(1)
    off = np.concatenate(([0], np.cumsum(hi - lo + 1)))
    assert off[-1] > (1 << 24) + (1 << 20)
    res, tabs = device_tables(eng, c)
    assert tabs.entries == off[-1]
    assert np.array_equal(tabs.lo.cpu().numpy()[0], lo) and np.array_equal(tabs.off.cpu().numpy(), off)
    import torch
    picks = np.unique(np.concatenate([rng.integers(0, off[-1], 2000), [0, off[1] - 1, off[G - 1], off[G] - 1]]))
    got = tabs.tab[torch.from_numpy(picks).to(eng.device)].cpu().numpy()
    gene = np.searchsorted(off, picks, side="right") - 1
    e2, var = res["e2"].cpu().numpy()[0], res["var"].cpu().numpy()[0]
    for e, g, u in zip(picks.tolist(), gene.tolist(), got.tolist()):
        r = S10.cmh(list(zip(a[g].tolist(), m[g].tolist(), k.tolist(), n.tolist())))
        assert (r["e2"], r["var"]) == (e2[g], var[g])
        assert u == S11.u_entry(int(lo[g]) + e - int(off[g]), r["e2"], r["var"]), (e, g)


# ---- 3. minima and counts ---------------------------------------------------------------------------------------
def spec_passes(c, spec, a_perm):
    """(minu [T, P], r_cmh_fwer [T, G], r_cmh_fwer_sd [T, G]) of the spec under the pooled counts a_perm [T, P, G]."""
    lo, off, tab = spec["lo"], spec["off"], spec["tab"]
    size = np.diff(off).reshape(c.T, c.G)
    assert (a_perm >= lo[:, None, :]).all() and (a_perm < (lo + size)[:, None, :]).all()     # a' inside [lo, hi]
    minu, r, r_sd = [], [], []
    for t in range(c.T):
        u_perm = S11.permuted(lo, off, tab, t, a_perm[t])
        mu, rt = S11.single_step(u_perm, spec["u_obs"][t])
        rs, q0 = S11.step_down(u_perm, spec["u_obs"][t])
        assert np.array_equal(q0, mu)
        minu.append(mu), r.append(rt), r_sd.append(rs)
    return np.stack(minu), np.stack(r), np.stack(r_sd)


@pytest.mark.parametrize("name,P", [("small", 200), ("wide", 64)])
def test_minima_and_counts_equal_the_spec(eng, name, P):
    c, spec = case_and_spec(eng, name)
    _bits, a_perm = c.labels(eng, P, SEED)
    want_minu, want_r, want_sd = spec_passes(c, spec, a_perm)
    res = eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=SEED, strata=c.sp, cmh=True, cmh_fwer=True,
                        cmh_stepdown=True)
    got = {k: res[k].cpu().numpy() for k in ("minu", "u_obs", "r_cmh_fwer", "r_cmh_fwer_sd", "r_cmh")}
    assert np.array_equal(got["u_obs"], spec["u_obs"]) and np.array_equal(got["minu"], want_minu)
    assert np.array_equal(got["r_cmh_fwer"], want_r) and np.array_equal(got["r_cmh_fwer_sd"], want_sd)
    r, r_sd, r_cmh = got["r_cmh_fwer"], got["r_cmh_fwer_sd"], got["r_cmh"].view(np.uint32).astype(np.int64)
    assert (r_sd <= r).all() and (r >= r_cmh).all() and (r < P).any()
    print("%s: %d of %d (trait, gene) pairs gain from the step-down" % (name, (r_sd < r).sum(), r.size))
    first = np.argmin(spec["u_obs"], axis=1)
    assert np.array_equal(r_sd[np.arange(c.T), first], r[np.arange(c.T), first])
    # the single-step pass on its own (k_permute_minp instead of the step-down's by-product)
    alone = eng.westfall_young(c.gm, c.trv, c.mkv, P, SEED, res, strata=c.sp, cmh_fwer=True)
    assert "minp" not in alone and "r_cmh_fwer_sd" not in alone
    assert np.array_equal(alone["minu"].cpu().numpy(), want_minu)
    assert np.array_equal(alone["r_cmh_fwer"].cpu().numpy(), want_r)
    # one trait per table group; three label batches
    assert eng.minp_trait_groups(res["counts"], 1) == [(t, t + 1) for t in range(c.T)]
    batch = -(-P // 3)
    label_budget = batch * c.T * eng.row_words(c.N) * 4
    assert eng.perm_batch(c.T, c.N, P, budget_bytes=label_budget) == batch and -(-P // batch) == 3
    for kw in ({"table_budget_bytes": 1}, {"label_budget_bytes": label_budget}):
        for single in (False, True):
            wy = eng.westfall_young(c.gm, c.trv, c.mkv, P, SEED, res, strata=c.sp, cmh_fwer=True,
                                    cmh_stepdown=not single, **kw)
            assert np.array_equal(wy["minu"].cpu().numpy(), want_minu), (kw, single)
            assert np.array_equal(wy["r_cmh_fwer"].cpu().numpy(), want_r), (kw, single)
            if not single:
                assert np.array_equal(wy["r_cmh_fwer_sd"].cpu().numpy(), want_sd), kw
    # the Fisher passes beside them are those of the call without the CMH flags
    both = eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=SEED, strata=c.sp, cmh=True, fwer=True,
                         stepdown=True, cmh_fwer=True, cmh_stepdown=True)
    fisher = eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=SEED, strata=c.sp, fwer=True, stepdown=True)
    for key in ("minp", "r_fwer", "r_fwer_sd", "r", "p"):
        assert np.array_equal(both[key].cpu().numpy(), fisher[key].cpu().numpy()), key
    for key in ("minu", "r_cmh_fwer", "r_cmh_fwer_sd"):
        assert np.array_equal(both[key].cpu().numpy(), got[key]), key


def test_one_gene_alone_counts_like_the_region(eng):
    """With a single gene the minimum over the genes is the gene's own u: r_cmh_fwer = r_cmh, except within half a
    count of the expectation, where the statistic is 0 and both are P."""
    from fractions import Fraction
    c, spec = case_and_spec(eng, "small")
    a, m, k, n = spec["amkn"]
    P, seen_near, seen_far = 200, 0, 0
    for g in (0, 1, 3, 5, 8, 13, 21, 34, 55, 89, 144, 299):
        one = Case(eng, c.genes[g:g + 1], c.traits, c.strata, S=c.S)
        res = eng.associate(one.gm, one.trv, one.mkv, permutations=P, seed=SEED, strata=one.sp, cmh=True,
                            cmh_fwer=True, cmh_stepdown=True)
        r = res["r_cmh_fwer"].cpu().numpy()[:, 0]
        r_cmh = res["r_cmh"].cpu().numpy().view(np.uint32)[:, 0]
        assert np.array_equal(res["r_cmh_fwer_sd"].cpu().numpy()[:, 0], r)
        assert np.array_equal(r, r_cmh), g
        for t in range(c.T):
            A, E, V = S10.exact(C.tables(a, m, k, n, t, g))
            near = V == 0 or abs(A - E) <= Fraction(1, 2)
            if near:
                assert r[t] == P and r_cmh[t] == P, (t, g)
            seen_near, seen_far = seen_near + near, seen_far + (not near)
    assert seen_near >= 3 and seen_far >= 10


# ---- 4. the cache -----------------------------------------------------------------------------------------------
def test_fisher_and_cmh_tables_do_not_meet_in_the_cache(eng):
    from scoary_amd.engine import AssociationEngine
    c, spec = case_and_spec(eng, "small")
    P = 96
    gm = eng.pack_dense(c.genes)
    plan = eng.trait_plan(c.trv, c.mkv, c.N)
    res = eng.associate(gm, c.trv, c.mkv, permutations=P, seed=SEED, strata=c.sp, cmh=True, plan=plan)
    first = eng.minp(gm, c.trv, c.mkv, P, SEED, plan=plan, strata=c.sp).cpu().numpy()
    assert set(gm.minp_caches) == {"fisher"} and gm.minp_cache["key"] is None
    fisher_tables = gm.minp_cache["tables"]
    wy = eng.westfall_young(gm, c.trv, c.mkv, P, SEED, res, plan=plan, strata=c.sp, cmh_fwer=True, cmh_stepdown=True)
    assert set(gm.minp_caches) == {"fisher", "cmh"} and gm.minp_caches["cmh"]["key"] is c.sp
    assert gm.minp_cache["tables"] is fisher_tables            # a slot per kind: the CMH pass evicts nothing
    kept = gm.minp_caches["cmh"]["tables"]
    assert kept is not fisher_tables and np.array_equal(kept.tab.cpu().numpy(), spec["tab"])
    again_cmh = eng.westfall_young(gm, c.trv, c.mkv, P, SEED, res, plan=plan, strata=c.sp, cmh_fwer=True)
    assert gm.minp_caches["cmh"]["tables"] is kept             # the same kind and strata plan: reused
    second = eng.minp(gm, c.trv, c.mkv, P, SEED, plan=plan, strata=c.sp).cpu().numpy()
    assert gm.minp_cache["tables"] is fisher_tables and np.array_equal(first, second) and (first < 1).any()
    # another strata plan of the same strata: the CMH tables are built again, Fisher's stay
    other = eng.strata_plan(c.strata, c.trv, c.mkv, c.N, S=c.S)
    res2 = eng.associate(gm, c.trv, c.mkv, permutations=P, seed=SEED, strata=other, cmh=True, plan=plan)
    wy2 = eng.westfall_young(gm, c.trv, c.mkv, P, SEED, res2, plan=plan, strata=other, cmh_fwer=True)
    assert gm.minp_caches["cmh"]["key"] is other and gm.minp_caches["cmh"]["tables"] is not kept
    assert gm.minp_cache["tables"] is fisher_tables
    assert np.array_equal(wy2["minu"].cpu().numpy(), wy["minu"].cpu().numpy())
    fresh = AssociationEngine(0)
    try:
        fc = Case(fresh, c.genes, c.traits, c.strata, S=c.S)
        want = fresh.associate(fc.gm, fc.trv, fc.mkv, permutations=P, seed=SEED, strata=fc.sp, cmh=True,
                               cmh_fwer=True, cmh_stepdown=True)
        for key in ("minu", "r_cmh_fwer", "r_cmh_fwer_sd"):
            assert np.array_equal(wy[key].cpu().numpy(), want[key].cpu().numpy()), key
        assert np.array_equal(again_cmh["minu"].cpu().numpy(), want["minu"].cpu().numpy())
    finally:
        fresh.close()


# ---- 5. the snap of E2 (step 2) -----------------------------------------------------------------------------------
SNAP_TABLES = [(3, 5, 4, 6), (1, 1, 2, 2), (0, 1, 0, 2), (1, 2, 5, 6)]          # (a, m, k, n): E = 6 exactly, A = 5


def snap_case():
    """The named counter-example of the spec as isolates -- a stratum's k positives first, the gene in the first a
    of them and in the first m - a of the negatives -- as gene 0, its complement as gene 1 (2E = 20 there), and a
    few random genes."""
    trait, strata, gene = [], [], []
    for s, (a, m, k, n) in enumerate(SNAP_TABLES):
        trait += [1] * k + [0] * (n - k)
        strata += [s] * n
        gene += [1] * a + [0] * (k - a) + [1] * (m - a) + [0] * (n - k - (m - a))
    gene = np.array(gene, dtype=np.uint8)
    rng = np.random.default_rng(16)
    genes = np.concatenate([gene[None], 1 - gene[None], (rng.random((6, len(gene))) < 0.5).astype(np.uint8)])
    return genes, np.array(trait, dtype=np.uint8)[None], np.array(strata)


def unsnapped_row(lo, hi, e2, var):
    """Step 3 WITHOUT step 2: what a table without the snap would hold."""
    delta = np.abs(np.arange(lo, hi + 1).astype(np.float64) - 0.5 * e2)
    y = np.minimum(0.5, delta)
    return 1.0 / (1.0 + ((delta - y) * (delta - y)) / var)


def test_the_snap_of_e2_on_the_device(eng):
    """An exact tie (2E an integer that the fp64 sum E2 misses): the device table holds the snapped values, bit for
    bit, and they differ from the un-snapped formula -- the two equally extreme counts carry the same u, so the
    tie is counted and r_cmh_fwer >= r_cmh holds where it would otherwise break."""
    genes, traits, strata = snap_case()
    c = Case(eng, genes, traits, strata, S=4)
    a, m, k, n = c.recount()
    assert C.tables(a, m, k, n, 0, 0) == SNAP_TABLES
    lo, off, tab, A = S11.csr(a, m, k, n)
    res, tabs = device_tables(eng, c)
    e2, var = res["e2"].cpu().numpy()[0], res["var"].cpu().numpy()[0]
    snapped = np.array([S11.snap(x) != x for x in e2])
    assert snapped[0] and e2[0] != 12.0 and S11.snap(e2[0]) == 12.0 and A[0, 0] == 5
    got = tabs.tab.cpu().numpy()
    assert np.array_equal(tabs.lo.cpu().numpy(), lo) and np.array_equal(tabs.off.cpu().numpy(), off)
    assert np.array_equal(got, tab)
    for g in np.flatnonzero(snapped):
        row = got[off[g]:off[g + 1]]
        raw = unsnapped_row(int(lo[0, g]), int(lo[0, g]) + len(row) - 1, e2[g], var[g])
        assert not np.array_equal(row, raw), g                  # a kernel without step 2 would write `raw`
    row = got[off[0]:off[1]]
    raw = unsnapped_row(int(lo[0, 0]), int(lo[0, 0]) + len(row) - 1, e2[0], var[0])
    at5, at7 = 5 - int(lo[0, 0]), 7 - int(lo[0, 0])
    assert row[at7] == row[at5] and raw[at7] != raw[at5]
    # tau itself: the entry points take e2 as an array, so values around an integer can be handed in directly --
    # 1e-6 away is snapped (<=), 1.5e-6 away is not
    import torch
    probe = np.array([12.0 + 1e-6, 12.0 - 1e-6, 12.0 + 1.5e-6, 12.0 - 1.5e-6, 11.5, e2[0]])
    want_snap = [S11.snap(x) != x for x in probe]
    assert want_snap == [True, True, False, False, False, True]
    G = len(probe)
    d_e2 = torch.from_numpy(probe).to(eng.device)
    d_var = torch.full((G,), float(var[0]), dtype=torch.float64, device=eng.device)
    d_off = torch.arange(0, 9 * (G + 1), 9, dtype=torch.int64, device=eng.device)          # nine entries per row
    d_lo = torch.full((1, G), 2, dtype=torch.int32, device=eng.device)
    d_tab = torch.zeros(9 * G, dtype=torch.float64, device=eng.device)
    eng._check(eng.lib.scoary_cmh_minp_fill(eng.h, eng._ptr(d_e2), eng._ptr(d_var), eng._ptr(d_off), eng._ptr(d_lo),
                                            1, G, 9 * G, eng._ptr(d_tab), eng._stream()), "scoary_cmh_minp_fill")
    filled = d_tab.cpu().numpy().reshape(G, 9)
    for g, x in enumerate(probe):
        assert np.array_equal(filled[g], S11.u_row(2, 10, float(x), float(var[0]))), g
        assert np.array_equal(filled[g], unsnapped_row(2, 10, float(x), float(var[0]))) != want_snap[g], g
    # the counts: the tie at x = 7 is in S10's region and in {u <= u_obs} alike
    P = 200
    out = eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=SEED, strata=c.sp, cmh=True, cmh_fwer=True,
                        cmh_stepdown=True)
    _bits, a_perm = c.labels(eng, P, SEED)
    assert (a_perm[0, :, 0] == 7).any() and (a_perm[0, :, 0] == 6).any()
    r, r_cmh = out["r_cmh_fwer"].cpu().numpy(), out["r_cmh"].cpu().numpy().view(np.uint32)
    assert (r >= r_cmh).all()
    u_perm = S11.permuted(lo, off, tab, 0, a_perm[0])
    want_minu, want_r = S11.single_step(u_perm, S11.observed(lo, off, tab, A)[0])
    assert np.array_equal(out["minu"].cpu().numpy()[0], want_minu) and np.array_equal(r[0], want_r)
    one = Case(eng, genes[:1], traits, strata, S=4)
    alone = eng.associate(one.gm, one.trv, one.mkv, permutations=P, seed=SEED, strata=one.sp, cmh=True, cmh_fwer=True)
    assert np.array_equal(alone["r_cmh_fwer"].cpu().numpy(), alone["r_cmh"].cpu().numpy().view(np.uint32))
    assert alone["r_cmh_fwer"].cpu().numpy()[0, 0] == ((a_perm[0, :, 0] <= 5) | (a_perm[0, :, 0] >= 7)).sum()


# ---- 6. refusals --------------------------------------------------------------------------------------------------
def test_the_entry_points_refuse_what_scoary_cmh_refuses(eng):
    """Return codes of scoary_cmh_minp_plan / _fill: the limits of the strata plan and T (SCOARY_ERR_SIZE), bad
    arguments (SCOARY_ERR_ARG); every refusal comes before anything is launched or written."""
    import ctypes
    import torch
    OK, ERR_ARG, ERR_SIZE = 0, -1, -3
    c, spec = case_and_spec(eng, "small")
    res, tabs = device_tables(eng, c)
    off, lo = tabs.off.clone(), tabs.lo.clone()
    tab = tabs.tab.clone()
    scratch = torch.zeros((int(eng.lib.scoary_cmh_scratch_bytes(c.N)) + 7) // 8, dtype=torch.int64, device=eng.device)
    entries = ctypes.c_int64(-7)
    max_s, max_n = eng.strata_max()

    def plan(G=c.G, T=c.T, N=c.N, S=c.S, tiled=c.gm.tiled, scratch_=scratch, out=entries):
        return eng.lib.scoary_cmh_minp_plan(
            eng.h, eng._ptr(tiled) if tiled is not None else None, eng._ptr(c.mkv), *eng._strata_ptrs(c.sp), G, T, N,
            S, eng._ptr(scratch_) if scratch_ is not None else None, eng._ptr(off), eng._ptr(lo),
            ctypes.byref(out) if out is not None else None, eng._stream())

    def fill(T=c.T, G=c.G, total=tabs.entries, e2=res["e2"]):
        return eng.lib.scoary_cmh_minp_fill(eng.h, eng._ptr(e2) if e2 is not None else None, eng._ptr(res["var"]),
                                            eng._ptr(off), eng._ptr(lo), T, G, total, eng._ptr(tab), eng._stream())

    assert plan(S=max_s + 1) == ERR_SIZE and b"strata" in eng.lib.scoary_last_error(eng.h)
    assert plan(N=max_n + 1) == ERR_SIZE and b"isolates" in eng.lib.scoary_last_error(eng.h)
    assert plan(T=65536) == ERR_SIZE and b"65535" in eng.lib.scoary_last_error(eng.h)
    for bad in (dict(G=0), dict(T=0), dict(N=0), dict(S=0), dict(tiled=None), dict(scratch_=None), dict(out=None)):
        assert plan(**bad) == ERR_ARG, bad
    assert fill(T=65536, total=1 << 40) == ERR_SIZE
    for bad in (dict(T=0), dict(G=0), dict(total=c.T * c.G - 1), dict(e2=None)):
        assert fill(**bad) == ERR_ARG, bad
    assert eng.lib.scoary_cmh_minp_plan(None, *[None] * 6, 1, 1, 1, 1, *[None] * 5) == ERR_ARG
    torch.cuda.synchronize()
    # nothing was written by a refused call
    assert entries.value == -7
    assert torch.equal(off, tabs.off) and torch.equal(lo, tabs.lo) and torch.equal(tab, tabs.tab)
    assert plan() == OK and entries.value == tabs.entries and fill() == OK
    torch.cuda.synchronize()
    assert torch.equal(off, tabs.off) and torch.equal(tab, tabs.tab)
    # engine level: a result and tables that do not belong together are an error, not a clamp
    with pytest.raises(ValueError, match="outside its gene's support"):
        eng.cmh_observed(tabs, res["a"] + 1000)
    with pytest.raises(ValueError, match="other traits or genes"):
        eng.cmh_observed(tabs, res["a"][:1])
