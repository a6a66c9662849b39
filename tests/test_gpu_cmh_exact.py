"""The exact conditional test over the strata (spec S12; scoary_cmh_exact) on the device: one stratum against
k_fisher, small strata against Fractions (tests/cmh_exact_spec.py), the boundaries of the running support, many tiny
strata, a p near 1e-190, the Monte-Carlo limit of r_cmh, the tables under the unchanged Westfall-Young kernels, and
the command line.  Bound everywhere: cmh_exact_spec.check -- 1e-12 absolute and relative, [0, 1e-290] below 1e-290."""
import csv
import io
import os
import sys

import numpy as np
import pytest

import cmh_cases as C
import cmh_exact_spec as S12
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


def run_exact(eng, c, tables=True):
    """(cmh()'s result, cmh_exact()'s result as numpy arrays; off / lo / tab with ``tables``)."""
    res = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    ex = eng.cmh_exact(c.gm, c.mkv, c.sp, res, tables=tables)
    out = {"p": ex["p"].cpu().numpy(), "p_region": ex["p_region"].cpu().numpy(), "a": res["a"].cpu().numpy(),
           "crit": res["crit"].cpu().numpy().view(np.uint32)}
    if tables:
        t = ex["tables"]
        out.update(off=t.off.cpu().numpy(), lo=t.lo.cpu().numpy(), tab=t.tab.cpu().numpy())
        assert t.entries == out["off"][-1] == len(out["tab"])
    return res, out


check_pairs = C.check_exact_pairs      # table, p (bit-identical to its table entry) and p_region against the reference


def all_pairs(c):
    return [(t, g) for t in range(c.T) for g in range(c.G)]


# ---- 1. one stratum is Fisher -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 600])
def test_one_stratum_is_fishers_exact_test(eng, N):
    genes, traits, _rng = C.random_genes_traits(300, N, 3, 1)
    assert (traits[2] == 2).any()
    c = Case(eng, genes, traits, np.zeros(N, dtype=np.int64), S=1)
    _res, got = run_exact(eng, c)
    fisher = eng.associate(c.gm, c.trv, c.mkv)["p"].cpu().numpy()
    err = np.abs(got["p"] - fisher)
    print("N = %d: exact p against k_fisher's, max abs error %.3e" % (N, err.max()))
    assert err.max() <= 1e-12
    plain, _ = run_exact(eng, c, tables=False)[1], None
    assert np.array_equal(plain["p"], got["p"]) and np.array_equal(plain["p_region"], got["p_region"])
    # Fisher's own tables (S7) hold the same numbers over the same supports
    ft = eng.minp_tables(eng.counts(c.gm, c.trv, c.mkv)[0])
    assert np.array_equal(ft.off.cpu().numpy(), got["off"]) and np.array_equal(ft.lo.cpu().numpy(), got["lo"])
    assert np.abs(ft.tab.cpu().numpy() - got["tab"]).max() <= 1e-12


def test_the_longest_support_and_one_isolate_more(eng):
    from scoary_amd import _abi
    N = eng.cmh_exact_max_isolates()
    assert N >= 8190
    rng = np.random.default_rng(N)
    genes = (rng.random((64, N + 1)) < 0.5).astype(np.uint8)
    traits = (rng.random((1, N + 1)) < 0.5).astype(np.uint8)
    c = Case(eng, genes[:, :N], traits[:, :N], np.zeros(N, dtype=np.int64), S=1)
    _res, got = run_exact(eng, c)
    assert np.diff(got["off"]).max() > 3900
    fisher = eng.associate(c.gm, c.trv, c.mkv)["p"].cpu().numpy()
    err = np.abs(got["p"] - fisher)
    print("N = %d: exact p against k_fisher's, max abs error %.3e" % (N, err.max()))
    assert err.max() <= 1e-12
    ft = eng.minp_tables(eng.counts(c.gm, c.trv, c.mkv)[0])
    assert np.array_equal(ft.off.cpu().numpy(), got["off"])
    S12.check(got["tab"], ft.tab.cpu().numpy(), "N = %d against Fisher's tables" % N)
    over = Case(eng, genes, traits, np.zeros(N + 1, dtype=np.int64), S=1)
    res = eng.cmh(over.gm, over.trv, over.mkv, over.sp)
    with pytest.raises(_abi.ScoaryHipError, match=r"more isolates than scoary_cmh_exact_max_isolates\(\) = %d" % N):
        eng.cmh_exact(over.gm, over.mkv, over.sp, res)


# ---- 2. small strata against Fractions ----------------------------------------------------------------------------
def test_edge_case_against_fractions(eng):
    genes, traits, strata, names = C.edge_case()
    c = Case(eng, genes, traits, strata, S=len(C.EDGE_NK))
    _res, got = run_exact(eng, c)
    check_pairs(c, got, all_pairs(c), "edge case")
    dead = np.diff(got["off"]).reshape(c.T, c.G) == 1
    assert dead.any() and (got["p"][dead] == 1.0).all() and (got["p_region"][dead] == 1.0).all()
    for name in ("none", "all"):
        assert dead[:, names.index(name)].all()


def test_graded_case_against_the_restatement(eng):
    """N = 6000, supports of 2600 entries: the exact reference costs seconds per pair here, so every pair is held to
    the floating-point restatement (itself within 1.1e-15 of the Fractions, test_cmh_exact_spec.py); p runs from
    3e-15 down through 1e-290 to 0."""
    genes, traits, strata = C.graded_case()
    c = Case(eng, genes, traits, strata, S=4)
    _res, got = run_exact(eng, c)
    check_pairs(c, got, all_pairs(c), "graded case", reference=S12.restate)
    p = got["p"][0]
    assert p[0] > 1e-20 and (p == 0).any() and ((p > 1e-280) & (p < 1e-100)).sum() > 10


@pytest.mark.parametrize("S", [2, 7, 33])
def test_random_strata_against_fractions(eng, S):
    N, G, T = 300, 200, 3
    genes, traits, rng = C.random_genes_traits(G, N, T, S)
    c = Case(eng, genes, traits, rng.integers(0, S, N), S=S)
    _res, got = run_exact(eng, c)
    check_pairs(c, got, all_pairs(c), "N = 300, S = %d" % S, allow_ties=T * G // 100)
    plain = run_exact(eng, c, tables=False)[1]
    assert np.array_equal(plain["p"], got["p"]) and np.array_equal(plain["p_region"], got["p_region"])


# ---- 3. boundaries of the running support -----------------------------------------------------------------------
def test_running_support_crosses_64_256_and_1024(eng):
    N, S, G, T = 2100, 3, 40, 2
    genes, traits, rng = C.random_genes_traits(G, N, T, S, dense_genes=True)
    strata = np.repeat(np.arange(S), (150, 600, 1350))[rng.permutation(N)]
    for s in range(S):                                       # trait 1 and gene 5: half of every stratum each, so the
        idx = np.flatnonzero(strata == s)                    # support has 75 + 300 + 675 + 1 entries
        traits[1, idx] = np.arange(len(idx)) < len(idx) // 2
        genes[5, idx] = np.arange(len(idx)) % 2
    c = Case(eng, genes, traits, strata, S=S)
    _res, got = run_exact(eng, c)
    sizes = np.diff(got["off"])
    assert sizes.max() == sizes[G + 5] == 1051 and sizes.min() == 1
    a, m, k, n = c.recount()
    first = np.minimum(k[:, None, :], m) - np.maximum(0, k[:, None, :] + m - n[:, None, :])     # [T, G, S]
    run = np.cumsum(first, axis=2) + 1
    for edge in (64, 256):
        assert (run[:, :, 0] < edge).any() and (run[:, :, 1:] > edge).any(), edge
    assert (run[1, 5] > np.array([64, 256, 1024])).all()
    check_pairs(c, got, C.subsample_pairs(T, G, 7) + [(1, 5)], "N = 2100, S = 3")
    # every table: 1 at a mode and p in (0, 1] -- but for the ends of the longest supports, whose true p lies below
    # the doubles (1e-400 at 1051 entries; S12 step 5 takes any value in [0, 1e-290] there): zeros at the ends only
    zeros = 0
    for i in range(T * G):
        row = got["tab"][got["off"][i]:got["off"][i + 1]]
        live = np.flatnonzero(row > 0)
        assert row.max() == 1.0 and row.min() >= 0.0 and len(live) == live[-1] - live[0] + 1
        assert row[live].min() < 1e-250 or len(live) == len(row)
        zeros += len(row) - len(live)
    print("N = 2100, S = 3: %d of %d table entries underflow to 0" % (zeros, len(got["tab"])))


# ---- 4. many tiny strata ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["contiguous", "random"])
def test_256_strata_of_8(eng, layout):
    N, S, G, T = 2048, 256, 30, 2
    genes, traits, rng = C.random_genes_traits(G, N, T, S)
    strata = np.repeat(np.arange(S), N // S)
    if layout == "random":
        strata = strata[rng.permutation(N)]
    c = Case(eng, genes, traits, strata, S=S)
    _res, got = run_exact(eng, c)
    assert np.diff(got["off"]).max() > 300
    check_pairs(c, got, C.subsample_pairs(T, G, 8), "S = 256, %s" % layout)


# ---- 5. deep tail -------------------------------------------------------------------------------------------------
def test_a_gene_equal_to_the_trait_inside_every_stratum(eng):
    N, S, G = 2000, 50, 6
    genes, traits, rng = C.random_genes_traits(G, N, 1, S)
    traits[0] = rng.random(N) < 0.075
    genes[0] = traits[0]
    c = Case(eng, genes, traits, rng.integers(0, S, N), S=S)
    _res, got = run_exact(eng, c)
    a, m, k, n = c.recount()
    _lo, _tab, p, region, tie = S12.reference(C.tables(a, m, k, n, 0, 0))
    print("deep tail: reference p %.6e, device %.6e; region %.6e, device %.6e"
          % (p, got["p"][0, 0], region, got["p_region"][0, 0]))
    assert 1e-290 <= p <= 1e-150 and not tie
    check_pairs(c, got, all_pairs(c), "deep tail")


# ---- 6. the Monte-Carlo limit -------------------------------------------------------------------------------------
_SEVEN = {}


def seven_strata(eng):
    if not _SEVEN:
        N, S, G, T = 300, 7, 100, 2
        genes, traits, rng = C.random_genes_traits(G, N, T, S)
        _SEVEN["c"] = Case(eng, genes, traits, rng.integers(0, S, N), S=S)
    return _SEVEN["c"]


def test_r_cmh_converges_to_the_region_mass(eng):
    c, P = seven_strata(eng), 20000
    res = eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=SEED, strata=c.sp, cmh=True, cmh_exact=True)
    r = res["r_cmh"].cpu().numpy().view(np.uint32).astype(np.float64)
    mass = res["cmh_exact_region_p"].cpu().numpy()
    _res, got = run_exact(eng, c, tables=False)
    assert np.array_equal(mass, got["p_region"]) and np.array_equal(res["cmh_exact_p"].cpu().numpy(), got["p"])
    dist = np.abs(r / P - mass)
    bound = 6.0 * np.sqrt(mass * (1.0 - mass) / P) + 1.0 / P
    print("Monte-Carlo limit: max |r / P - p_region| / bound = %.3f" % (dist / bound).max())
    assert (dist <= bound).all()
    plain = eng.associate(c.gm, c.trv, c.mkv, permutations=64, seed=SEED, strata=c.sp, cmh=True)
    assert "cmh_exact_p" not in plain


# ---- 7. tables drive the existing kernels -------------------------------------------------------------------------
def test_westfall_young_over_exact_p(eng):
    c, P = seven_strata(eng), 256
    res, got = run_exact(eng, c)
    source = eng.cmh_exact_source(c.gm, c.mkv, c.sp, res)
    assert source.kind == "cmh_exact" and source.key is c.sp
    import torch
    observed = torch.empty((c.T, c.G), dtype=torch.float64, device=eng.device)
    minp = eng.minp(c.gm, c.trv, c.mkv, P, SEED, strata=c.sp, source=source, observed_out=observed).cpu().numpy()
    assert np.array_equal(observed.cpu().numpy(), got["p"])
    _bits, a_perm = c.labels(eng, P, SEED)
    want_sd = []
    for t in range(c.T):
        p_perm = S11.permuted(got["lo"], got["off"], got["tab"], t, a_perm[t])
        want, r = S11.single_step(p_perm, got["p"][t])
        assert np.array_equal(minp[t], want)
        want_sd.append(S11.step_down(p_perm, got["p"][t])[0])
    r_sd, by_product = eng.minp_stepdown(c.gm, c.trv, c.mkv, P, SEED, strata=c.sp, source=source)
    assert np.array_equal(by_product.cpu().numpy(), minp)
    assert np.array_equal(r_sd.cpu().numpy(), np.stack(want_sd))
    assert (minp < 1).all() and len(np.unique(minp)) > 20


# ---- 8. command line ----------------------------------------------------------------------------------------------
def _run_cli(argv, outdir, trait):
    from scoary_amd import methods as m
    old = sys.argv
    sys.argv = ["scoary"] + argv + ["-o", str(outdir), "--no-time"]
    try:
        with pytest.raises(SystemExit) as e:
            m.main()
        assert e.value.code in (0, None), e.value.code
    finally:
        sys.argv = old
    with open(os.path.join(str(outdir), trait + ".results.csv"), newline="") as f:
        text = f.read()
    return text, list(csv.reader(io.StringIO(text)))


def test_cli_column_is_last_and_holds_the_engines_values(eng, tmp_path):
    from scoary_amd import methods as m
    from scoary_amd.engine import pack_bits_rows
    N, G, S = 90, 40, 4
    rng = np.random.default_rng(90)
    genes = (rng.random((G, N)) < rng.uniform(0.1, 0.9, (G, 1))).astype(np.uint8)
    trait = (rng.random(N) < 0.4).astype(np.uint8)
    strata = rng.integers(0, S, N)
    strains = ["iso%03d" % i for i in range(N)]
    gpa, tr, sf = (os.path.join(str(tmp_path), f) for f in ("genes.csv", "traits.csv", "strata.csv"))
    with open(gpa, "w") as f:
        f.write(",".join(["Gene", "Non-unique Gene name", "Annotation"] + ["c%d" % i for i in range(11)] + strains) + "\n")
        for g in range(G):
            f.write(",".join(["gene%03d" % g, "", "hypothetical"] + [""] * 11 +
                             [("g%d_%d" % (g, i) if v else "") for i, v in enumerate(genes[g])]) + "\n")
    with open(tr, "w") as f:
        f.write(",resistance\n" + "".join("%s,%d\n" % (s, v) for s, v in zip(strains, trait)))
    with open(sf, "w") as f:
        f.write("Isolate,Lineage\n" + "".join("%s,L%d\n" % (s, v) for s, v in zip(strains, strata)))
    base = ["-g", gpa, "-t", tr, "--no_pairwise", "-p", "1.0", "--cmh", sf]
    old_text, old = _run_cli(base, tmp_path / "old", "resistance")
    _text, new = _run_cli(base + ["--cmh-exact"], tmp_path / "new", "resistance")
    assert new[0] == old[0] + ["CMH_exact_p"] and [r[:-1] for r in new] == old and len(old) > 10
    idx, _labels = m.strata_indices(m.read_strata_file(sf), strains)
    c = Case(m.get_engine(), genes, trait[None], idx)
    _res, got = run_exact(m.get_engine(), c, tables=False)
    for d in new[1:]:
        g = int(d[0][4:])
        assert d[-1] == repr(float(got["p"][0, g])), d[0]
    assert len({d[-1] for d in new[1:]}) > 10
    again_text, _rows = _run_cli(base, tmp_path / "again", "resistance")
    assert again_text == old_text and "CMH_exact" not in old_text
