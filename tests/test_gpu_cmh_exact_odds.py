"""The conditional maximum-likelihood odds ratio over the strata and its exact confidence limits (spec S13;
scoary_cmh_exact_odds) on the device.  Every (trait, gene) of a case is held to the floating-point restatement
(tests/cmh_exact_odds_spec.py: bisection, no kernel code) at 1e-12 relative, and up to 200 sampled pairs with supports
of at most 600 entries to the exact bracketing check in integers at 1e-12 instead; 0, +inf and nan must match exactly.
Pairs with f(A) < 1e-290 are outside the specification: there the values must be non-negative and not nan."""
import csv
import io
import os
import sys

import numpy as np
import pytest

import cmh_cases as C
import cmh_exact_spec as S12
from cmh_cases import Case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def run_odds(eng, c, level=0.95):
    """cmh_exact_odds() of a case as a float64 [3, T, G] numpy array (odds, lower, upper) and cmh()'s a."""
    res = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    od = eng.cmh_exact_odds(c.gm, c.mkv, c.sp, res, level=level)
    got = np.stack([od[k].cpu().numpy() for k in ("odds", "lower", "upper")])
    assert got.shape == (3, c.T, c.G) and got.dtype == np.float64
    return got, res["a"].cpu().numpy()


def check_case(c, got, a_dev, level, what, pairs=None):
    """cmh_cases.check_odds_case, and that the exact check took part wherever a support allowed it."""
    seen, exact = C.check_odds_case(c, got, a_dev, level, what, pairs)
    assert exact > 0 or min(seen["L"]) > 600 or max(seen["L"]) == 1
    return seen


# ---- 1. one stratum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 600])
def test_one_stratum(eng, N):
    genes, traits, _rng = C.random_genes_traits(149, N, 3, 1)
    assert (traits[2] == 2).any() and genes.shape[0] % 4
    c = Case(eng, genes, traits, np.zeros(N, dtype=np.int64), S=1)
    got, a_dev = run_odds(eng, c)
    seen = check_case(c, got, a_dev, 0.95, "one stratum, N = %d" % N)
    assert seen["nan"] >= 6 and max(seen["L"]) > N // 6                     # genes 1 and 2: a single support point


# ---- 2. edges ---------------------------------------------------------------------------------------------------
def test_edges_of_the_support_and_a_trait_without_positives(eng):
    genes, traits, strata, names = C.edge_case()
    traits = np.concatenate([traits, np.zeros((1, traits.shape[1]), dtype=np.uint8)])      # npos = 0
    genes = np.concatenate([genes, (traits[0] == 1)[None].astype(np.uint8)])               # the trait itself
    c = Case(eng, genes, traits, strata, S=len(C.EDGE_NK))
    got, a_dev = run_odds(eng, c)
    seen = check_case(c, got, a_dev, 0.95, "edge case")
    assert seen["zero"] > 0 and seen["inf"] > 0 and seen["nan"] >= c.G
    assert np.isnan(got[0, 2]).all() and (got[1, 2] == 0).all() and (got[2, 2] == np.inf).all()      # npos = 0
    for name in ("none", "all"):                                            # a single support point
        col = names.index(name)
        assert np.isnan(got[0, :, col]).all() and (got[1, :, col] == 0).all() and (got[2, :, col] == np.inf).all()
    own = got[:, 0, c.G - 1]                                                 # A = hi inside every stratum
    assert own[0] == np.inf and own[2] == np.inf and 1.0 < own[1] < np.inf
    assert got[0, 0, names.index("odds_inf")] == np.inf


# ---- 3. random strata -------------------------------------------------------------------------------------------
_RANDOM = {}


@pytest.mark.parametrize("level", [0.5, 0.95, 0.999])
@pytest.mark.parametrize("S", [2, 7, 33])
def test_random_strata(eng, S, level):
    if S not in _RANDOM:
        genes, traits, rng = C.random_genes_traits(150, 300, 2, S)
        _RANDOM[S] = Case(eng, genes, traits, rng.integers(0, S, 300), S=S)
    c = _RANDOM[S]
    got, a_dev = run_odds(eng, c, level)
    check_case(c, got, a_dev, level, "N = 300, S = %d" % S)


# ---- 4. long supports -------------------------------------------------------------------------------------------
def test_running_support_crosses_64_256_and_1024(eng):
    N, S, G, T = 2100, 3, 40, 2
    genes, traits, rng = C.random_genes_traits(G, N, T, S, dense_genes=True)
    strata = np.repeat(np.arange(S), (150, 600, 1350))[rng.permutation(N)]
    for s in range(S):                                       # trait 1 and gene 5: half of every stratum each, so the
        idx = np.flatnonzero(strata == s)                    # support has 75 + 300 + 675 + 1 entries
        traits[1, idx] = np.arange(len(idx)) < len(idx) // 2
        genes[5, idx] = np.arange(len(idx)) % 2
    c = Case(eng, genes, traits, strata, S=S)
    got, a_dev = run_odds(eng, c)
    seen = check_case(c, got, a_dev, 0.95, "N = 2100, S = 3")
    sizes = np.array(seen["L"])
    assert sizes.max() == sizes[G + 5] == 1051 and sizes.min() == 1
    for edge in (64, 256, 1024):                             # more than one entry per lane, more than one wavefront
        assert (sizes < edge).any() and (sizes > edge).any(), edge


def test_the_longest_support_and_one_isolate_more(eng):
    from scoary_amd import _abi
    N = eng.cmh_exact_max_isolates()
    assert N == 8190
    rng = np.random.default_rng(N)
    trait = np.zeros(N + 1, dtype=np.uint8)
    trait[:N // 2] = 1                                       # k = 4095 of the first 8190
    genes = np.zeros((6, N + 1), dtype=np.uint8)
    for g, overlap in enumerate((2047, 2048, 2030, 2075, 2000, 2110)):       # m = 4095, observed near the centre
        genes[g, rng.permutation(N // 2)[:overlap]] = 1
        genes[g, N // 2 + rng.permutation(N // 2)[:N // 2 - overlap]] = 1
    c = Case(eng, genes[:, :N], trait[None, :N], np.zeros(N, dtype=np.int64), S=1)
    got, a_dev = run_odds(eng, c)
    seen = check_case(c, got, a_dev, 0.95, "N = %d, m = k = 4095" % N)
    assert seen["L"] == [4096] * 6 and seen["unspecified"] == 0 and np.isfinite(got).all() and (got > 0).all()
    _lo, f = S12.float_pmf([(2047, 4095, 4095, 8190)])
    assert f[0] == 0.0 and f[-1] == 0.0 and (f == 0).sum() > 1000            # the tails of f are exactly 0
    over = Case(eng, genes, trait[None], np.zeros(N + 1, dtype=np.int64), S=1)
    res = eng.cmh(over.gm, over.trv, over.mkv, over.sp)
    with pytest.raises(_abi.ScoaryHipError, match=r"scoary_cmh_exact_odds: more isolates than "
                                                  r"scoary_cmh_exact_max_isolates\(\) = %d" % N):
        eng.cmh_exact_odds(over.gm, over.mkv, over.sp, res)


# ---- 5. many strata ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["contiguous", "random"])
def test_256_strata_of_8(eng, layout):
    N, S, G, T = 2048, 256, 30, 2
    genes, traits, rng = C.random_genes_traits(G, N, T, S)
    strata = np.repeat(np.arange(S), N // S)
    if layout == "random":
        strata = strata[rng.permutation(N)]
    c = Case(eng, genes, traits, strata, S=S)
    got, a_dev = run_odds(eng, c)
    seen = check_case(c, got, a_dev, 0.95, "S = 256, %s" % layout)
    assert max(seen["L"]) > 300


def test_more_than_one_stratum_per_lane(eng):
    N, S, G, T = 2400, 300, 20, 2
    genes, traits, rng = C.random_genes_traits(G, N, T, S)
    c = Case(eng, genes, traits, np.repeat(np.arange(S), N // S)[rng.permutation(N)], S=S)
    got, a_dev = run_odds(eng, c)
    seen = check_case(c, got, a_dev, 0.95, "S = 300")
    assert max(seen["L"]) > 300


# ---- 6. strong association --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(10, 8), (60, 4)])
def test_strong_association_next_to_the_ends_of_the_support(eng, k, m):
    """N = 2000 in 10 strata of 200 with k positives each.  Gene 0 is carried by m positives of every stratum but for
    one carrier moved to a negative (A = hi - 1), gene 1 by m negatives but for one moved to a positive (A = lo + 1),
    genes 2 and 3 are the same without the move (A = hi, A = lo): psi from 0.0014 to 2e5, f(A) down to 1e-121."""
    S, size = 10, 200
    N = S * size
    strata = np.repeat(np.arange(S), size)
    trait = np.tile((np.arange(size) < k).astype(np.uint8), S)
    genes = np.zeros((4, N), dtype=np.uint8)
    for s in range(S):
        base = s * size
        genes[[0, 2], base:base + m] = 1                     # m of the positives
        genes[[1, 3], base + k:base + k + m] = 1             # m of the negatives
    genes[0, 0], genes[0, size - 1] = 0, 1
    genes[1, k], genes[1, 0] = 0, 1
    c = Case(eng, genes, trait[None], strata, S=S)
    got, a_dev = run_odds(eng, c)
    seen = check_case(c, got, a_dev, 0.95, "strong association, k = %d, m = %d" % (k, m))
    assert seen["L"] == [S * m + 1] * 4 and seen["unspecified"] == 0
    assert list(a_dev[0]) == [S * m - 1, 1, S * m, 0]
    assert got[0, 0, 0] > 50 and got[0, 0, 1] < 0.3 and got[0, 0, 2] == np.inf and got[0, 0, 3] == 0.0
    assert got[1, 0, 2] > 10 and got[2, 0, 3] < 1.0


# ---- 7. command line --------------------------------------------------------------------------------------------
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


def _cli_files(tmp_path):
    """A gene table of 40 genes x 90 isolates, one trait and a strata file of 4 strata under ``tmp_path``: (the three
    paths, genes, trait, strata, the isolates' names)."""
    N, G, S = 90, 40, 4
    rng = np.random.default_rng(91)
    genes = (rng.random((G, N)) < rng.uniform(0.1, 0.9, (G, 1))).astype(np.uint8)
    trait = (rng.random(N) < 0.4).astype(np.uint8)
    strata = rng.integers(0, S, N)
    genes[7] = trait                                         # A = hi: inf, and CMH_odds_ratio is inf too
    genes[8] = strata == 1                                   # a single support point: nan in both columns
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
    return (gpa, tr, sf), genes, trait, strata, strains


def test_cli_columns_are_the_last_and_hold_the_engines_values(eng, tmp_path):
    from scoary_amd import methods as m
    (gpa, tr, sf), genes, trait, _strata, strains = _cli_files(tmp_path)
    base = ["-g", gpa, "-t", tr, "--no_pairwise", "-p", "1.0", "--cmh", sf, "--cmh-exact"]
    old_text, old = _run_cli(base, tmp_path / "old", "resistance")
    names = ["CMH_exact_odds_ratio", "CMH_exact_odds_ratio_lower", "CMH_exact_odds_ratio_upper"]
    _text, new = _run_cli(base + ["--cmh-exact-odds", "--cmh-exact-level", "0.9"], tmp_path / "new", "resistance")
    assert new[0] == old[0] + names and [r[:-3] for r in new] == old and len(old) > 10
    assert old[0][-1] == "CMH_exact_p"
    idx, _labels = m.strata_indices(m.read_strata_file(sf), strains)
    c = Case(m.get_engine(), genes, trait[None], idx)
    got, _a = run_odds(m.get_engine(), c, 0.9)
    mh = new[0].index("CMH_odds_ratio")
    met = set()
    for d in new[1:]:
        g = int(d[0][4:])
        assert d[-3:] == [repr(float(v)) for v in got[:, 0, g]], d[0]
        if d[-3] in ("inf", "nan"):
            assert d[mh] == d[-3], d[0]                      # spelled as CMH_odds_ratio spells them
            met.add(d[-3])
    assert met == {"inf", "nan"} and len({d[-3] for d in new[1:]}) > 10
    default_text, default = _run_cli(base + ["--cmh-exact-odds"], tmp_path / "default", "resistance")
    got95, _a = run_odds(m.get_engine(), c)
    assert [d[-3:] for d in default[1:]] == [[repr(float(v)) for v in got95[:, 0, int(d[0][4:])]] for d in default[1:]]
    assert [d[-3] for d in default[1:]] == [d[-3] for d in new[1:]] and default_text != _text      # the level is used
    again_text, _rows = _run_cli(base, tmp_path / "again", "resistance")
    assert again_text == old_text and "CMH_exact_odds" not in old_text


def test_cli_every_optional_flag_at_once_writes_the_columns_of_each_flag_alone(eng, tmp_path):
    """associate()'s "every other result is that of the same call without the option, bit for bit", seen at the file:
    every column of a run with all six optional flags has the cell texts of the run that had only its flag."""
    from scoary_amd import methods as m
    (gpa, tr, sf), _genes, _trait, _strata, _strains = _cli_files(tmp_path)
    base = ["-g", gpa, "-t", tr, "--no_pairwise", "-p", "1.0", "--cmh", sf, "-e", "100"]
    flags = {"--permute-fwer": ["Westfall_Young_p"], "--permute-fwer-stepdown": ["Westfall_Young_stepdown_p"],
             "--cmh-fwer": ["CMH_Westfall_Young_p"], "--cmh-fwer-stepdown": ["CMH_Westfall_Young_stepdown_p"],
             "--cmh-exact": ["CMH_exact_p"],
             "--cmh-exact-odds": ["CMH_exact_odds_ratio", "CMH_exact_odds_ratio_lower", "CMH_exact_odds_ratio_upper"]}
    _text, plain = _run_cli(base, tmp_path / "plain", "resistance")
    _text, full = _run_cli(base + list(flags), tmp_path / "full", "resistance")
    # the header: the columns of the base run and the eight of the flags, the optional ones in OPTIONAL_COLUMNS' order
    # (so the Westfall-Young columns of the Fisher statistic stand before --cmh's own, not behind the base header)
    added = [name for names in flags.values() for name in names]
    optional = [name for name, _key, _count in m.OPTIONAL_COLUMNS]
    assert len(added) == 8 and [c for c in full[0] if c not in added] == plain[0]
    assert full[0] == [c for c in plain[0] if c not in optional] + optional
    assert len(full) == len(plain) > 10

    def column(table, name):
        return [row[table[0].index(name)] for row in table[1:]]
    for name in plain[0]:
        assert column(full, name) == column(plain, name), name
    for flag, names in flags.items():
        _text, alone = _run_cli(base + [flag], tmp_path / flag.strip("-"), "resistance")
        assert [c for c in alone[0] if c not in names] == plain[0] and set(names) <= set(alone[0]), flag
        for name in alone[0]:
            assert column(full, name) == column(alone, name), (flag, name)
        assert all(len(set(column(alone, name))) > 1 for name in names), flag       # (the cells are values)
