"""The Breslow-Day / Tarone test of homogeneity over the strata (spec S14; scoary_cmh_homogeneity) on the device.
Every (trait, gene) of a case is held to the floating-point restatement (tests/cmh_homog_spec.py, no kernel code) fed
with the per-stratum counts of numpy and the odds ratio the device itself wrote: both statistics and df bit for bit,
p within 1e-10 relative of the restatement's tail at the device's own statistic and df."""
import csv
import io
import os
import sys

import numpy as np
import pytest

import cmh_cases as C
import cmh_homog_spec as S14
import cmh_spec as S10
from args_cases import good_strata_file
from cmh_cases import Case
from conftest import golden_text, read_dense

pytestmark = pytest.mark.gpu
SEED = 1973


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def run_homog(eng, c):
    """cmh_homogeneity() of a case as numpy arrays, and the odds ratios of cmh() it read."""
    res = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    h = eng.cmh_homogeneity(c.gm, c.trv, c.mkv, c.sp, res)
    got = {k: v.cpu().numpy() for k, v in h.items()}
    assert set(got) == {"stat_bd", "stat_tarone", "p", "df"}
    for k, v in got.items():
        assert v.shape == (c.T, c.G) and v.dtype == (np.int32 if k == "df" else np.float64), k
    return got, res["odds"].cpu().numpy()


check_case = C.check_homog_case      # both statistics and df bit for bit, p within 1e-10 relative of the restatement


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------
def build_case(eng, name):
    if name == "interleaved":                    # a quad tail (257 isolates = 2 quads + 1 word) and missing values
        genes, traits, _rng = C.random_genes_traits(300, 257, 3, 4)
        assert (traits[2] == 2).any()
        return Case(eng, genes, traits, np.arange(257) % 4, S=4)
    if name == "singletons":                     # strata of one isolate, emptied strata, a stratum without members
        genes, traits, rng = C.random_genes_traits(130, 129, 2, 40)
        strata = rng.integers(0, 40, 129)
        strata[strata == 5] = 6                                               # index 5: no member
        for s, i in ((11, 0), (12, 64), (39, 128)):                           # one isolate each
            strata[strata == s] = 13
            strata[i] = s
        traits[1, strata == 20] = 2                                           # emptied for trait 1
        traits[:, strata == 21] = 2                                           # emptied for both
        assert not (strata == 5).any() and (strata == 12).sum() == 1 and (strata == 20).sum() > 1
        return Case(eng, genes, traits, strata, S=40)
    if name == "contiguous":                     # boundaries inside words
        genes, traits, _rng = C.random_genes_traits(200, 2100, 2, 7)
        sizes = (45, 610, 3, 333, 700, 409 - 30, 30)
        assert sum(sizes) == 2100 and all(sum(sizes[:i]) % 32 for i in range(1, 7))
        return Case(eng, genes, traits, np.repeat(np.arange(7), sizes), S=7)
    if name == "traits33":                       # the trait tail of the last block
        genes, traits, rng = C.random_genes_traits(64, 96, 33, 3)
        return Case(eng, genes, traits, rng.integers(0, 3, 96), S=3)
    assert name == "one_stratum"
    genes, traits, _rng = C.random_genes_traits(70, 90, 2, 1)
    return Case(eng, genes, traits, np.zeros(90, dtype=np.int64), S=1)


@pytest.mark.parametrize("name", ["interleaved", "singletons", "contiguous", "traits33", "one_stratum"])
def test_kernel_against_the_restatement(eng, name):
    c = build_case(eng, name)
    got, odds = run_homog(eng, c)
    defined, undefined, _df = check_case(c, got, odds, name)
    if name == "one_stratum":                    # L <= 1 everywhere
        assert defined == 0 and undefined == c.T * c.G
    else:
        assert defined > c.G and undefined >= 2 * c.T                        # genes 1 and 2: psi = nan


# ---- 2. the edge genes ------------------------------------------------------------------------------------------
def test_edge_genes(eng):
    genes, traits, strata, names = S14.edge_case()
    c = Case(eng, genes, traits, strata, S=len(S14.EDGE_NK))
    got, odds = run_homog(eng, c)
    defined, undefined, _df = check_case(c, got, odds, "edge genes")
    col = names.index
    assert odds[0, col("psi_one")] == 1.0 and got["df"][0, col("psi_one")] == 1
    assert odds[0, col("psi_zero")] == 0.0 and odds[0, col("psi_inf")] == np.inf
    for name in ("none", "all", "psi_zero", "psi_inf", "one_stratum"):       # genes in no and in every isolate among them
        for t in (0, 1):
            assert got["df"][t, col(name)] == 0 and got["p"][t, col(name)] == 1.0, name
            assert np.isnan(got["stat_bd"][t, col(name)]) and np.isnan(got["stat_tarone"][t, col(name)]), name
    assert np.isnan(odds[:, col("none")]).all() and np.isnan(odds[:, col("all")]).all()
    assert got["df"][:, col("masked")].tolist() == [3, 1] and got["df"][0, col("with_n_one")] == 2
    assert got["df"][0, col("b_negative")] == 1 and got["df"][0, col("psi_above_one")] == 2
    assert defined >= 6 and undefined >= 10


# ---- 3. the anchor ----------------------------------------------------------------------------------------------
def test_ucb_admissions_on_the_device(eng):
    gene, trait, strata = [], [], []
    for s, (a, b, c_, d) in enumerate(S10.UCB.values()):
        gene += [1] * a + [0] * b + [1] * c_ + [0] * d
        trait += [1] * (a + b) + [0] * (c_ + d)
        strata += [s] * (a + b + c_ + d)
    assert len(gene) == 4526
    c = Case(eng, np.array([gene], dtype=np.uint8), np.array([trait], dtype=np.uint8), np.array(strata), S=6)
    got, odds = run_homog(eng, c)
    check_case(c, got, odds, "UCBAdmissions")
    want = S14.UCB_ANCHOR
    assert odds[0, 0] == want["psi"] and got["df"][0, 0] == 5
    assert (got["stat_bd"][0, 0], got["stat_tarone"][0, 0]) == S14.homogeneity(S10.tables_abcd(S10.UCB.values()),
                                                                               want["psi"])[:2]
    assert abs(got["stat_bd"][0, 0] - want["bd"]) <= 1e-12 * want["bd"]
    assert abs(got["stat_tarone"][0, 0] - want["tarone"]) <= 1e-12 * want["tarone"]
    assert abs(got["p"][0, 0] - want["p"]) <= 1e-10 * want["p"]


# ---- 4. the largest shape ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["interleaved", "blocked"])
def test_limit_shape(eng, layout):
    genes, traits, strata = C.limit_case(layout)
    c = Case(eng, genes, traits, strata, S=C.LIMIT_S)
    assert (c.N, c.S, c.T, c.G) == (20479, 1024, 5, 40)
    got, odds = run_homog(eng, c)
    top = int(got["df"].max())
    pairs = set(C.subsample_pairs(c.T, c.G)) | {(int(t), int(g)) for t, g in zip(*np.nonzero(got["df"] == top))}
    _defined, _undefined, top_df = check_case(c, got, odds, "limit, %s" % layout, sorted(pairs))
    # interleaved: strata of 20 isolates, nearly all of them informative; blocked: of 2 to 33, most of them
    assert top_df == top >= 500


# ---- 5. associate -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 100])
def test_associate(eng, P):
    c = build_case(eng, "interleaved")
    kw = dict(permutations=P, seed=SEED, use_lists=False, strata=c.sp, cmh=True)
    res = eng.associate(c.gm, c.trv, c.mkv, cmh_homogeneity=True, **kw)
    res = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}
    got, _odds = run_homog(eng, c)
    assert np.array_equal(res["cmh_homog_p"], got["p"]) and np.array_equal(res["cmh_homog_df"], got["df"])
    assert np.array_equal(res["cmh_homog_stat"], got["stat_tarone"], equal_nan=True)
    assert (got["df"] > 0).any() and (got["p"] < 1.0).any()
    plain = eng.associate(c.gm, c.trv, c.mkv, **kw)
    assert set(res) == set(plain) | {"cmh_homog_p", "cmh_homog_stat", "cmh_homog_df"}
    for key, v in plain.items():
        if hasattr(v, "cpu"):
            assert np.array_equal(res[key], v.cpu().numpy(), equal_nan=v.is_floating_point()), key
        else:
            assert res[key] is v or res[key] == v, key
    with pytest.raises(ValueError, match="cmh_homogeneity=True needs cmh=True"):
        eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=SEED, use_lists=False, strata=c.sp,
                      cmh_homogeneity=True)


# ---- 6. command line --------------------------------------------------------------------------------------------
def _run_cli(argv, outdir):
    from scoary_amd import methods as m
    old = sys.argv
    sys.argv = ["scoary"] + argv + ["-o", str(outdir), "--no-time"]
    try:
        with pytest.raises(SystemExit) as e:
            m.main()
        assert e.value.code in (0, None), e.value.code
    finally:
        sys.argv = old
    with open(os.path.join(str(outdir), "Tetracycline_resistance.results.csv"), newline="") as f:
        text = f.read()
    return text, list(csv.reader(io.StringIO(text)))


def planted_table(exampledir, tmp_path):
    """A copy of the example gene table with one more gene: the trait itself in stratum 0 (L0 of good_strata_file), its
    complement in stratum 1 and every second isolate of stratum 2 -- opposite effects that cancel in the common odds
    ratio.  (path, text)."""
    with open(os.path.join(exampledir, "Gene_presence_absence.csv"), newline="") as f:
        text = f.read()
    trait_rows = list(csv.reader(io.StringIO(golden_text("exampledata/Tetracycline_resistance.csv.gz"))))
    value = {r[0]: r[1] for r in trait_rows[1:]}
    lines = text.splitlines()
    header = next(csv.reader([lines[0]]))
    cells = ["planted_gene", "", "planted"] + [""] * 11
    for i, s in enumerate(header[14:]):
        on = value[s] == "1" if i % 3 == 0 else value[s] == "0" if i % 3 == 1 else (i // 3) % 2 == 0
        cells.append("x" if on else "")
    path = os.path.join(str(tmp_path), "planted.csv")
    text = "\n".join(lines + [",".join('"%s"' % cell for cell in cells)]) + "\n"
    with open(path, "w") as f:
        f.write(text)
    return path, text


@pytest.mark.parametrize("more", [[], ["--permute", "100", "--cmh-exact"]])
def test_cli_column_is_the_last_and_holds_the_engines_values(eng, exampledir, tmp_path, more):
    from scoary_amd import methods as m
    from scoary_amd.engine import pack_bits_rows
    sf = good_strata_file(exampledir, tmp_path)
    gpa, gpa_text = planted_table(exampledir, tmp_path)
    base = ["-g", gpa, "-t", os.path.join(exampledir, "Tetracycline_resistance.csv"), "--no_pairwise", "-p", "1.0",
            "--cmh", sf] + more
    old_text, old = _run_cli(base, tmp_path / "old")
    _text, new = _run_cli(base + ["--cmh-homogeneity"], tmp_path / "new")
    assert new[0] == old[0] + ["CMH_homogeneity_p"] and [r[:-1] for r in new] == old and len(old) > 10
    assert old[0][-1] == ("CMH_exact_p" if more else "CMH_odds_ratio")
    assert ",".join('"%s"' % cell for cell in new[1][:-1]) == old_text.splitlines()[1]        # byte for byte
    # the engine, called directly on the same table and strata
    ids, strains, genes, _names, traits = read_dense(gpa_text, golden_text("exampledata/Tetracycline_resistance.csv.gz"))
    idx, _labels = m.strata_indices(m.read_strata_file(sf), strains)
    c = Case(m.get_engine(), genes, traits, idx)
    got, _odds = run_homog(m.get_engine(), c)
    mh = new[0].index("CMH_odds_ratio")
    spelled = set()
    for d in new[1:]:
        g = ids.index(d[0])
        assert d[-1] == repr(float(got["p"][0, g])), d[0]
        assert float(d[-1]) == got["p"][0, g] or d[-1] == "nan"
        if d[mh] == "nan":
            spelled.add(d[-1])
    assert spelled <= {"1.0"} and len({d[-1] for d in new[1:]}) > 10
    (planted,) = [d for d in new[1:] if d[0] == "planted_gene"]
    assert float(planted[new[0].index("CMH_p")]) > 0.05 and float(planted[-1]) < 1e-3, planted
    again_text, _rows = _run_cli(base, tmp_path / "again")
    assert again_text == old_text and "CMH_homogeneity_p" not in old_text
