"""Randomised cross-checks of the stratified half of the library (specs S7 to S14), one case per call with fixed
seeds, in the style of stress_cases.py: label rows and tiles shuffled within strata (A), k_cmh and the exact-test
family that hangs on its result (B), the exceedance counts of associate(strata=, cmh=True) (C), the Westfall-Young
passes over the three kinds of table (D) and the matrix-core routing under strata (E).  The reference of every family
is a plain-Python restatement under tests/ or numpy on downloaded labels; none shares code with the library.

``draw(case, pools)`` makes the problem of a case and needs no engine, so tests/test_strata_stress_corpus.py draws the
identical corpora on the CPU and shows from the references alone what they reach.  tests/test_gpu_strata_stress.py
runs the families under `pytest -m gpu`.  A helper, not a test.

Every family function takes (eng, case) and returns (ok, description)."""
import types

import numpy as np

import cmh_cases as C
import cmh_exact_spec as S12
import cmh_spec as S10
import cmh_wy_spec as S11

SMALL_N = [1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 129, 257, 300, 511, 700]
WIDE_ONLY = [2047, 2048, 2049, 2559, 2560, 5200]     # the matrix cores' K-step limit, the list kernel's tile widths
WIDE_N = SMALL_N + WIDE_ONLY
S_POOL = [1, 2, 3, 7, 33, 64, 255, 256, 257, 300, 1024]
LAYOUTS = ("random", "blocked", "interleaved", "skewed")
G_POOL = [1, 3, 63, 65, 130]
LEVELS = (0.5, 0.95, 0.999)

# Per family: the seed, the pools a draw picks from and the number of cases the GPU test runs.  B: the references of the
# p table and of the odds ratio are exact arithmetic, so N comes from SMALL_N -- but no N <= 700 has 256 informative
# strata (a stratum needs two isolates at the least, and at N = 700 and S = 300 a random trait and gene leave about
# 120 strata with 0 < k < n and 0 < m < n), so every fourth case of B draws N from WIDE_ONLY and holds the p table to
# the floating-point restatement (cmh_exact_spec.restate, within 1.1e-15 of the Fractions: test_cmh_exact_spec.py)
# as test_gpu_cmh_exact.py::test_graded_case_against_the_restatement does.
POOLS = {
    "A": dict(seed=9001, N=SMALL_N, G=[1], P=[1, 31, 33, 65], cases=16),
    "B": dict(seed=9143, N=SMALL_N, G=G_POOL, P=[0], cases=16, wide_every=4),
    "C": dict(seed=9003, N=WIDE_N, G=G_POOL, P=[1, 64, 65, 200], cases=16),
    "D": dict(seed=9401, N=WIDE_N, G=G_POOL, P=[10, 64, 130], cases=10),
    "E": dict(seed=9005, N=[n for n in WIDE_N if n <= 2048], G=[33, 300, 513], P=[1, 64, 65, 193], cases=16),
}
B_TALLY = {"pairs": 0, "ties": 0}                    # family B's p comparisons and the near ties left out of them


def draw_strata(rng, layout, N, S):
    """Stratum indices int64 [N] in [0, S) of a layout; S may exceed N."""
    if layout == "interleaved":
        return np.arange(N, dtype=np.int64) % S
    if layout == "random":
        return rng.integers(0, S, N)
    if layout == "blocked":
        return np.sort(rng.integers(0, S, N))
    assert layout == "skewed"                        # one or two large strata and a tail of singletons
    big = rng.choice(S, size=min(S, int(rng.integers(1, 3))), replace=False)
    strata = big[rng.integers(0, len(big), N)].astype(np.int64)
    others = np.setdiff1d(np.arange(S), big)
    tail = min(N // 3, len(others))
    if tail:
        strata[rng.choice(N, size=tail, replace=False)] = rng.choice(others, size=tail, replace=False)
    return strata


def draw(case, pools):
    """The problem of ``case`` under ``pools`` (an entry of POOLS): a namespace of N, S, layout, G, T, P, base, level,
    seed, genes uint8 [G, N], traits uint8 [T, N] (2 = missing), strata int64 [N], and what the traits were given --
    ``emptied`` {trait: strata masked away altogether} and ``constant`` (the trait that is constant inside every
    stratum, or None).  Where G > 4, gene 1 follows trait 0 (nine isolates in ten), gene G - 3 is the complement of
    gene 0, gene G - 2 is in every isolate and gene G - 1 in none; the gene that follows a trait is what puts an exact p
    below 1e-20 into the corpus, which carrier frequencies drawn independently of the traits never do.  Gene 2 is
    carried by half of trait 0's valid isolates in every stratum that has an even number of them and by none in the
    others: every stratum's pmf is then symmetric, so is their convolution, and every count ties EXACTLY with its
    mirror image -- in doubles the two differ in their last bits, which is what the gamma of S12 step 3 is for."""
    rng = np.random.default_rng([pools["seed"], case])
    N = int(rng.choice(pools["N"]))
    if pools.get("wide_every") and case % pools["wide_every"] == pools["wide_every"] - 1:
        N = int(rng.choice(WIDE_ONLY))
    S = int(rng.choice(S_POOL))
    layout = str(rng.choice(LAYOUTS))
    G = int(rng.choice(pools["G"]))
    T = int(rng.integers(1, 6))
    P = int(rng.choice(pools["P"]))
    base = 32 * int(rng.integers(0, 32))
    level = float(rng.choice(LEVELS))
    seed = int(rng.integers(1, 1 << 62))
    strata = draw_strata(rng, layout, N, S)
    traits = (rng.random((T, N)) < rng.uniform(0.05, 0.95, (T, 1))).astype(np.uint8)
    live, emptied = np.unique(strata), {}
    for t in range(T):
        if rng.random() < 0.5:
            traits[t, rng.random(N) < rng.uniform(0.0, 0.3)] = 2
            if rng.random() < 0.5:
                gone = rng.choice(live, size=min(len(live), int(rng.integers(1, 3))), replace=False)
                traits[t, np.isin(strata, gone)] = 2
                emptied[t] = sorted(int(s) for s in gone)
    constant = None
    if rng.random() < 0.1:
        constant = int(rng.integers(0, T))
        traits[constant] = (rng.random(S) < 0.5).astype(np.uint8)[strata]
        emptied.pop(constant, None)
    genes = (rng.random((G, N)) < rng.uniform(0.0, 1.0, (G, 1))).astype(np.uint8)
    if G > 4:
        genes[1] = np.where(rng.random(N) < 0.9, traits[0] == 1, rng.random(N) < 0.5)
        genes[G - 3], genes[G - 2], genes[G - 1] = 1 - genes[0], 1, 0
        genes[2] = 0
        valid0 = traits[0] != 2
        for s in np.unique(strata[valid0]):
            idx = np.flatnonzero(valid0 & (strata == s))
            if len(idx) % 2 == 0:
                genes[2, idx[:len(idx) // 2]] = 1
    return types.SimpleNamespace(case=case, N=N, S=S, layout=layout, G=G, T=T, P=P, base=base, level=level, seed=seed,
                                 genes=genes, traits=traits, strata=strata, emptied=emptied, constant=constant)


def describe(family, pr):
    return "%s case %d: N=%d S=%d %s G=%d T=%d P=%d%s%s%s" % (
        family, pr.case, pr.N, pr.S, pr.layout, pr.G, pr.T, pr.P, " missing" if (pr.traits == 2).any() else "",
        " emptied=%s" % pr.emptied if pr.emptied else "",
        " constant=%d" % pr.constant if pr.constant is not None else "")


def _verdict(family, pr, check):
    """(ok, description) of a case whose checks are the assertions of ``check()``."""
    what = describe(family, pr)
    try:
        check()
    except AssertionError as e:
        return False, "%s -- %s" % (what, str(e)[:400])
    return True, what


# -- A: stratified label rows and tiles -----------------------------------------------------------------------------
def tile_bits(eng, tiles, T, N, P):
    """Label tiles (N <= 20479: one segment) -> ([T, P, N] 0/1, True when the zero row and the padding columns are
    0)."""
    lanes = eng.list_params(N)[0]
    tperm = lanes * 32
    ntiles = -(-P // tperm)
    tw = int(eng.lib.scoary_list_tile_words(N))
    t = tiles.cpu().numpy().view(np.uint32)[:T * ntiles * tw].reshape(T, ntiles, tw)
    t = t[:, :, :(N + 1) * lanes].reshape(T, ntiles, N + 1, lanes)
    out, clean = np.zeros((T, P, N), dtype=np.uint8), True
    for ti in range(T):
        for tile in range(ntiles):
            b = np.unpackbits(np.ascontiguousarray(t[ti, tile]).view(np.uint8), axis=1, bitorder="little")
            lo, hi = tile * tperm, min(P, tile * tperm + tperm)
            clean = clean and not b[N].any() and not b[:N, hi - lo:].any()
            out[ti, lo:hi] = b[:N, :hi - lo].T
    return out, clean


def labels_case(eng, case):
    """perm_generate(strata=) == strata_spec.s9_labels bit for bit, every permutation of the case; the tiles of
    perm_generate_tiles(strata=) == the transposed rows, zero row and zero padding included."""
    from strata_spec import s9_labels
    pr = draw(case, POOLS["A"])

    def check():
        c = C.Case(eng, pr.genes, pr.traits, pr.strata, S=pr.S)
        margins = eng.trait_plan(c.trv, c.mkv, pr.N).margins
        raw = eng.perm_generate(c.mkv, margins, pr.N, pr.P, pr.base, pr.seed, strata=c.sp).cpu().numpy().view(np.uint32)
        assert not raw[:, :, 2 * ((pr.N + 63) // 64):].any(), "padding words of the rows"
        bits = np.unpackbits(raw.view(np.uint8).reshape(pr.T, pr.P, -1), axis=2, bitorder="little")
        assert not bits[:, :, pr.N:].any(), "padding bits of the rows"
        rows = bits[:, :, :pr.N]
        tiles = eng.perm_generate_tiles(c.mkv, margins, pr.N, pr.P, pr.base, pr.seed, strata=c.sp)
        tiles, clean = tile_bits(eng, tiles, pr.T, pr.N, pr.P)
        assert clean, "zero row or padding columns of the tiles"
        assert np.array_equal(tiles, rows), "tiles != transposed rows"
        valid, lab, strata = (pr.traits != 2).astype(int), (pr.traits == 1).astype(int), pr.strata.tolist()
        for t in range(pr.T):
            for i in range(pr.P):
                want = s9_labels(pr.seed, t, pr.base + i, valid[t].tolist(), lab[t].tolist(), strata, pr.S)
                assert rows[t, i].tolist() == want, "row of trait %d, permutation %d" % (t, pr.base + i)
    return _verdict("A base=%d" % pr.base, pr, check)


# -- B: CMH and what hangs on its result ----------------------------------------------------------------------------
def b_genes(pr):
    """The genes of a B case that are held to the per-pair references: sixteen spread over the matrix and, where the
    draw has them, the gene that follows trait 0, the gene of exact ties, gene 0, its complement, the core gene and the
    absent gene."""
    sel = set(np.unique(np.linspace(0, pr.G - 1, 16).astype(np.int64)).tolist())
    if pr.G > 4:
        sel |= {0, 1, 2, pr.G - 3, pr.G - 2, pr.G - 1}
    return sorted(sel)


def b_pairs(pr):
    """The (trait, gene) pairs of a B case that take the costly references (p table, odds ratio): about sixteen of the
    pairs of b_genes, and the pairs of trait 0 with the gene that follows it, the gene of exact ties and gene 0's
    complement."""
    every = [(t, g) for g in b_genes(pr) for t in range(pr.T)]
    pairs = set(every[::max(1, len(every) // 16)])
    if pr.G > 4:
        pairs |= {(0, 1), (0, 2), (0, pr.G - 3), (pr.T - 1, pr.G - 1)}
    return sorted(pairs)


def b_exact(pr):
    """True where the p tables of the case are held to the Fractions, False where to the floating-point restatement."""
    return pr.N <= max(SMALL_N)


def cmh_case(eng, case):
    """One eng.cmh, then cmh_exact(tables=True), cmh_exact_odds and cmh_homogeneity, each at the bound its fixed-shape
    test holds it to (cmh_cases.check_cmh / check_exact_pairs / check_odds_case / check_homog_case).  The per-stratum
    margins and the pooled count are held to numpy for every pair, the per-pair references run over b_genes / b_pairs:
    the Python references of all 2890 pairs of the corpus take 16 s before the exact check of the odds ratios is
    added."""
    pr = draw(case, POOLS["B"])

    def check():
        c = C.Case(eng, pr.genes, pr.traits, pr.strata, S=pr.S)
        res = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
        out = {k: v.cpu().numpy() for k, v in res.items()}
        a, m, k, n = c.recount()
        assert np.array_equal(c.sp.smargins.cpu().numpy(), np.stack([k, n], axis=2)), "per-stratum margins"
        assert np.array_equal(out["a"], (a * (n > 0)[:, None, :]).sum(2)), "pooled counts"
        gsel = b_genes(pr)
        C.check_cmh({key: v[:, gsel] for key, v in out.items()}, C.restate(a[:, gsel], m[:, gsel], k, n))
        pairs = b_pairs(pr)
        ex = eng.cmh_exact(c.gm, c.mkv, c.sp, res, tables=True)
        got = {"p": ex["p"].cpu().numpy(), "p_region": ex["p_region"].cpu().numpy(), "a": out["a"],
               "crit": out["crit"].view(np.uint32), "off": ex["tables"].off.cpu().numpy(),
               "lo": ex["tables"].lo.cpu().numpy(), "tab": ex["tables"].tab.cpu().numpy()}
        assert ex["tables"].entries == got["off"][-1] == len(got["tab"])
        lean = eng.cmh_exact(c.gm, c.mkv, c.sp, res)
        assert np.array_equal(lean["p"].cpu().numpy(), got["p"]), "p without the tables"
        assert np.array_equal(lean["p_region"].cpu().numpy(), got["p_region"]), "p_region without the tables"
        B_TALLY["pairs"] += len(pairs) if b_exact(pr) else 0
        B_TALLY["ties"] += C.check_exact_pairs(c, got, pairs, describe("B", pr), allow_ties=len(pairs),
                                               reference=S12.reference if b_exact(pr) else S12.restate)
        od = eng.cmh_exact_odds(c.gm, c.mkv, c.sp, res, level=pr.level)
        C.check_odds_case(c, np.stack([od[key].cpu().numpy() for key in ("odds", "lower", "upper")]), out["a"],
                          pr.level, describe("B", pr), pairs)
        h = eng.cmh_homogeneity(c.gm, c.trv, c.mkv, c.sp, res)
        C.check_homog_case(c, {key: v.cpu().numpy() for key, v in h.items()}, out["odds"], describe("B", pr),
                           [(t, g) for t in range(pr.T) for g in gsel])
    return _verdict("B level=%s" % pr.level, pr, check)


# -- C: counts under stratified permutations ------------------------------------------------------------------------
def region_counts(crit, a_perm):
    """#{permutations whose pooled count lies in the region}: crit uint32 [T, G, 2], a_perm int64 [T, P, G] -> [T, G]
    (cmh_spec.in_region, the test the permutation kernels make, on whole arrays)."""
    c = crit.astype(np.int64)
    return S10.in_region((c[:, None, :, 0], c[:, None, :, 1]), a_perm).sum(1).astype(np.uint32)


def _poison(ws):
    """0xFF bytes in every buffer of a workspace that a step is meant to write before it reads."""
    for buf in (ws.scratch, ws.tiles, ws.perms, ws.lcrit, ws.bfrag, ws.r):
        if buf is not None:
            buf.fill_(-1)


def counts_case(eng, case):
    """associate(permutations=P, strata=sp, cmh=True), list-driven and dense: r and r_cmh == the host recount from the
    downloaded stratified labels, the float32 product and the regions the step itself reports."""
    pr = draw(case, POOLS["C"])

    def check():
        c = C.Case(eng, pr.genes, pr.traits, pr.strata, S=pr.S)
        _bits, a_perm = c.labels(eng, pr.P, pr.seed)
        eng.build_lists(c.gm)
        for use_lists in (True, False):
            ws = eng.workspace(c.gm, pr.T, pr.P, use_lists=use_lists)
            _poison(ws)
            res = eng.associate(c.gm, c.trv, c.mkv, permutations=pr.P, seed=pr.seed, use_lists=use_lists,
                                strata=c.sp, cmh=True, workspace=ws)
            for key, crit in (("r", "crit"), ("r_cmh", "cmh_crit")):
                got = res[key].cpu().numpy().view(np.uint32)
                want = region_counts(res[crit].cpu().numpy().view(np.uint32), a_perm)
                assert np.array_equal(got, want), "%s, use_lists=%s: %d of %d pairs differ" % (
                    key, use_lists, (got != want).sum(), want.size)
    return _verdict("C", pr, check)


# -- D: Westfall-Young over the three kinds of table ----------------------------------------------------------------
def d_budgets(eng, pr):
    """The budgets of a D case: every fifth case from 1 cuts the tables into one trait per group, every fifth from 3
    cuts the labels into two batches."""
    if pr.case % 5 == 1:
        return {"table_budget_bytes": 1}
    if pr.case % 5 == 3:
        return {"label_budget_bytes": -(-pr.P // 2) * pr.T * eng.row_words(pr.N) * 4}
    return {}


def d_traits(pr):
    """A D case whose table budget forces two trait groups has two traits at the least."""
    if pr.case % 5 == 1 and pr.T < 2:
        pr.traits = np.concatenate([pr.traits, 1 - (pr.traits & 1)])
        pr.T = 2
    return pr


def westfall_young_case(eng, case):
    """minp() and minp_stepdown() with strata, over Fisher's tables, the CMH tables and the exact tables: the minima
    and the step-down counts == cmh_wy_spec.permuted / single_step / step_down over the device's tables and the
    downloaded labels."""
    import torch
    pr = d_traits(draw(case, POOLS["D"]))

    def check():
        c = C.Case(eng, pr.genes, pr.traits, pr.strata, S=pr.S)
        kw = d_budgets(eng, pr)
        if "table_budget_bytes" in kw:
            assert len(eng.minp_trait_groups(eng.counts(c.gm, c.trv, c.mkv)[0], 1)) == pr.T >= 2
        if "label_budget_bytes" in kw:
            assert -(-pr.P // eng.perm_batch(pr.T, pr.N, pr.P, budget_bytes=kw["label_budget_bytes"])) == 2
        _bits, a_perm = c.labels(eng, pr.P, pr.seed)
        res = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
        sources = (eng.fisher_source(eng.counts(c.gm, c.trv, c.mkv)[0]), eng.cmh_source(c.gm, c.mkv, c.sp, res),
                   eng.cmh_exact_source(c.gm, c.mkv, c.sp, res))
        for source in sources:
            tabs = source.build(0, pr.T)
            lo, off, tab = tabs.lo.cpu().numpy(), tabs.off.cpu().numpy(), tabs.tab.cpu().numpy()
            observed = torch.empty((pr.T, pr.G), dtype=torch.float64, device=eng.device)
            minp = eng.minp(c.gm, c.trv, c.mkv, pr.P, pr.seed, strata=c.sp, source=source, observed_out=observed,
                            **kw).cpu().numpy()
            obs = observed.cpu().numpy()
            if source.kind != "fisher":
                assert np.array_equal(obs, S11.observed(lo, off, tab, res["a"].cpu().numpy().astype(np.int64)))
            r_sd, by_product = eng.minp_stepdown(c.gm, c.trv, c.mkv, pr.P, pr.seed, strata=c.sp, source=source, **kw)
            assert np.array_equal(by_product.cpu().numpy(), minp), "%s: the step-down's minima" % source.kind
            r_sd = r_sd.cpu().numpy()
            for t in range(pr.T):
                u = S11.permuted(lo, off, tab, t, a_perm[t])
                want, _r = S11.single_step(u, obs[t])
                assert np.array_equal(minp[t], want), "%s: minima of trait %d" % (source.kind, t)
                assert np.array_equal(r_sd[t], S11.step_down(u, obs[t])[0]), "%s: step-down of trait %d" % (
                    source.kind, t)
    return _verdict("D" + {1: " (a table group per trait)", 3: " (two label batches)"}.get(pr.case % 5, ""), pr, check)


# -- E: matrix-core routing under strata ----------------------------------------------------------------------------
def mfma_case(eng, case):
    """set_mfma_route("all") against "none" with strata and cmh: identical r and r_cmh, and the "none" result == the
    host recount on 16 genes."""
    pr = draw(case, POOLS["E"])

    def check():
        c = C.Case(eng, pr.genes, pr.traits, pr.strata, S=pr.S)
        eng.build_lists(c.gm)
        got = {}
        try:
            for mode in ("all", "none"):
                eng.set_mfma_route(mode)
                assert eng.mfma_split(c.gm, pr.T, pr.P) == (pr.G if mode == "all" else 0), "routing %s" % mode
                res = eng.associate(c.gm, c.trv, c.mkv, permutations=pr.P, seed=pr.seed, use_lists=True, strata=c.sp,
                                    cmh=True)
                got[mode] = {key: res[key].cpu().numpy().view(np.uint32).copy()
                             for key in ("r", "r_cmh", "crit", "cmh_crit")}
        finally:
            eng.set_mfma_route("auto")
        for key in ("r", "r_cmh"):
            assert np.array_equal(got["all"][key], got["none"][key]), "%s: %d of %d pairs differ between the routes" % (
                key, (got["all"][key] != got["none"][key]).sum(), got["none"][key].size)
        gsel = np.unique(np.linspace(0, pr.G - 1, 16).astype(np.int64))
        a_perm = C.pooled_counts(c.label_rows(eng, pr.P, pr.seed), pr.genes[gsel])
        for key, crit in (("r", "crit"), ("r_cmh", "cmh_crit")):
            assert np.array_equal(got["none"][key][:, gsel], region_counts(got["none"][crit][:, gsel], a_perm)), key
    return _verdict("E", pr, check)


FAMILIES = {"A": labels_case, "B": cmh_case, "C": counts_case, "D": westfall_young_case, "E": mfma_case}
