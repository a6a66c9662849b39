"""--categorical-strata FILE: the refusals on the command line (they exit before the engine is touched) and in
Gcmh_results (the same rules as ValueErrors), and what the feature adds beside the pinned tables, the binding and the
build."""
import os

import pytest

from args_cases import good_rows, good_strata_file as _strata_file, run_refused as _run, strains as _strains, strata_file

FLAG = "--categorical-strata"
CATEGORICAL = ("Cannot use --categorical-strata without --categorical. Its strata are those of the generalized "
               "Cochran-Mantel-Haenszel test of the categorical traits")


def _cfile(exampledir, tmp_path):
    path = os.path.join(str(tmp_path), "c.csv")
    with open(path, "w") as f:
        f.write("Name,host\n" + "".join("%s,%s\n" % (s, "ab"[i % 2]) for i, s in enumerate(_strains(exampledir))))
    return path


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.categorical_strata is None
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", "--categorical", "c.csv", FLAG,
                                         "s.csv", "-e", "50"])
    assert (args.categorical, args.categorical_strata, args.permute) == ("c.csv", "s.csv", 50)


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    c = _cfile(exampledir, tmp_path)
    strata = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run(["--no_pairwise", FLAG, strata]) == CATEGORICAL
    assert run([FLAG, strata]) == CATEGORICAL
    # the rules of --categorical come first
    assert run([FLAG, strata, "--categorical", c]).startswith("Cannot use --categorical without --no_pairwise")
    assert run(["--no_pairwise", "--categorical", c, FLAG, strata, "-e", "100", "--permute-strata", strata]).startswith(
        "Cannot use --categorical together with --permute-strata")
    missing = os.path.join(str(tmp_path), "nowhere.csv")
    assert run(["--no_pairwise", "--categorical", c, FLAG, missing]) == \
        "Could not find the strata file of --categorical-strata: " + missing
    many = strata_file(tmp_path, [(s, "L%d" % i) for i, s in enumerate(_strains(exampledir))], name="many.csv")
    from scoary_amd import _abi
    monkeypatch.setattr(_abi, "PERM_MAX_STRATA", 5)
    n = len(_strains(exampledir))
    assert run(["--no_pairwise", "--categorical", c, FLAG, many]) == \
        "The strata file %s names %d strata for the analysed isolates; --categorical-strata takes at most 5" % (many, n)
    monkeypatch.undo()
    short = strata_file(tmp_path, good_rows(exampledir)[3:], name="short.csv")
    assert run(["--no_pairwise", "--categorical", c, FLAG, short]).startswith(
        "The strata file does not name a stratum for 3 of the analysed isolates")
    assert run(["--no_pairwise", "--categorical", c, FLAG, strata, "-e", "5"]) == \
        "The absolute minimum number of permutations is 10 (or 0 to deactivate)"


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import dist, methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    labels = [["a", "b", None]]
    for kw, text in ((dict(no_pairwise=False), "categorical traits need no_pairwise"),
                     (dict(collapse=True), "categorical traits exclude collapse")):
        with pytest.raises(ValueError, match=text):
            m.Gcmh_results(None, ["x"], labels, [0, 0, 1], **kw)
    with pytest.raises(ValueError, match="categorical trait sero has 9 classes, at most 8 are taken: merge rare classes"):
        m.Gcmh_results(None, ["sero"], [[str(i % 9) for i in range(10)]], [0] * 10)
    monkeypatch.setattr(dist, "world_rank", lambda: (4, 1))
    with pytest.raises(ValueError, match="categorical traits need a single process"):
        m.Gcmh_results(None, ["x"], labels, [0, 0, 1])
    assert list(m.GCMH_TEXT) == ["categorical", "file", "strata"] and m.GCMH_TEXT["categorical"] == CATEGORICAL


def test_most_enriched_class_is_the_largest_ratio_to_the_expectation_and_prefers_the_first():
    from scoary_amd import methods as m
    assert m.most_enriched_expected([1, 2, 0, 2], [2.0, 4.0, 0.0, 3.0]) == 3
    assert m.most_enriched_expected([1, 2], [2.0, 4.0]) == 0                   # a tie goes to the first class
    assert m.most_enriched_expected([5, 0, 5], [0.0, 7.0, 9.0]) == 2           # a class that expects none is never it
    assert m.most_enriched_expected([0, 0], [1.5, 2.5]) == 0


def test_the_feature_is_beside_the_pinned_tables_and_in_the_build():
    import __graft_entry__ as ge
    from scoary_amd import _abi, engine, methods as m
    assert not any("gcmh" in name.lower() for name, _k, _c in m.ALL_COLUMNS)
    assert not any(rule.flag == FLAG for rule in m.ALL_RULES)
    assert m.GCMH_COLUMNS == ("Number_with_gene", "Number_without_gene", "Carriers_by_class", "Expected_by_class",
                              "Most_enriched_class", "GCMH", "GCMH_df", "GCMH_p", "Bonferroni_p", "Benjamini_H_p")
    for name in ("scoary_gcmh_form_doubles", "scoary_gcmh", "scoary_permute_gcmh"):
        assert name in _abi.SIGNATURES
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert _abi.ABI_VERSION == 11 and "spec S21" in header and engine.GCMH_FORM == 35
    for name in ("gcmh_plan", "gcmh", "gcmh_rows", "gcmh_permute"):
        assert callable(getattr(engine.AssociationEngine, name))
    assert any(s.endswith("scoary_gcmh.hip") for s in ge.HIP_SRCS)
    # both translation units compile the one text of the class planes' walk and of the chi-square tail
    csrc = os.path.dirname(ge.HIP_SRCS[0])
    for unit in ("scoary_categorical.hip", "scoary_gcmh.hip"):
        with open(os.path.join(csrc, unit)) as f:
            text = f.read()
        assert '#include "scoary_cat_planes.hpp"' in text and '#include "scoary_chi2.hpp"' in text
        assert "void cat_count(" not in text and "double chi2_tail(" not in text
    assert [r["name"] for r in ge.GCMH_RULES] == ["k_gcmh_observed", "k_gcmh_permute"]
    names = ["_ZN12_GLOBAL__N_115k_gcmh_observedEPK15HIP_vector_typeIjLj4EEl", "_ZN12_GLOBAL__N_114k_gcmh_permuteEPKjl"]
    ok = {n: {"VGPRs": 90, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0} for n in names}
    ge.check_kernel_resources(ok, ge.GCMH_RULES)
    for n in names:                                   # scratch or a spill in either kernel fails the build
        for field, what in (("ScratchSize", "scratch 64"), ("SGPRs Spill", "SGPR spills 64"), ("VGPRs Spill", "VGPR spills 64")):
            bad = {k: dict(v, **({field: 64} if k == n else {})) for k, v in ok.items()}
            with pytest.raises(RuntimeError, match=what):
                ge.check_kernel_resources(bad, ge.GCMH_RULES)
    every = (ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES +
             ge.CMH_HOMOG_RULES + ge.FISHER_CHAINS_RULES + ge.RANKSUM_RULES + ge.VANELTEREN_RULES + ge.RANK_WY_RULES +
             ge.RANK_SD_RULES + ge.RANK_SHIFT_RULES + ge.CATEGORICAL_RULES)
    for other in every:                               # and the new names are in no other family
        assert not any(other["name"] in n and not (other["exclude"] and other["exclude"] in n) for n in names)
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            ge.check_kernel_resources(json.load(f), ge.GCMH_RULES)
