"""--categorical FILE: the refusals on the command line (they exit before the engine is touched) and in
Categorical_results (the same rules as ValueErrors), the ninth class, the reader of the file, and what the feature
adds beside the pinned tables, the binding and the build."""
import os

import pytest

from args_cases import good_strata_file as _strata_file, run_refused as _run, strains as _strains

FLAG = "--categorical"
NO_PAIRWISE = ("Cannot use --categorical without --no_pairwise. The chi-square test is a population structure-naive "
               "test of every gene")
COLLAPSE = ("Cannot use --categorical together with --collapse. The chi-square test is a test of every gene of the "
            "table")
STRATA = ("Cannot use --categorical together with --permute-strata. The labels are shuffled over all isolates with a "
          "label; a shuffle within strata is not implemented")
RANKS = "Cannot use --categorical under more than one rank: the test runs over all genes in a single process"
CLASSES = ("Cannot use --categorical with the trait %s: it has %d classes among the analysed isolates, the test takes "
           "at most 8. Merge rare classes into one before the run")


def _cfile(tmp_path, text="Name,host\nA,pig\n", name="c.csv"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.categorical is None
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", FLAG, "c.csv", "-e", "50"])
    assert args.categorical == "c.csv" and args.permute == 50 and args.no_pairwise


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    from scoary_amd import dist
    c = _cfile(tmp_path)
    strata = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run([FLAG, c]) == NO_PAIRWISE
    assert run([FLAG, c, "--collapse"]) == NO_PAIRWISE                          # in this order
    assert run(["--no_pairwise", FLAG, c, "--collapse"]) == COLLAPSE
    assert run(["--no_pairwise", FLAG, c, "-e", "100", "--permute-strata", strata]) == STRATA
    assert run(["--no_pairwise", FLAG, c, "--collapse", "-e", "100", "--permute-strata", strata]) == COLLAPSE
    missing = os.path.join(str(tmp_path), "nowhere.csv")
    assert run(["--no_pairwise", FLAG, missing]) == "Could not find the categorical traits file: " + missing
    assert run(["--no_pairwise", FLAG, c, "-e", "5"]) == \
        "The absolute minimum number of permutations is 10 (or 0 to deactivate)"
    monkeypatch.setattr(dist, "world_rank", lambda: (2, 0))
    assert run(["--no_pairwise", FLAG, c]) == RANKS


def test_a_ninth_class_refuses_the_run_on_the_command_line(exampledir, tmp_path, monkeypatch):
    """Nine classes among the analysed isolates refuse the run and name the trait; nine classes of which one belongs
    to an isolate the analysis does not hold are eight."""
    iso = _strains(exampledir)
    assert len(iso) >= 18
    rows = ["%s,c%d,%s\n" % (s, i % 9, "ab"[i % 2]) for i, s in enumerate(iso)]
    nine = _cfile(tmp_path, "Name,serotype,pair\n" + "".join(rows), "nine.csv")
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run(["--no_pairwise", FLAG, nine]) == CLASSES % ("serotype", 9)
    rows = ["%s,c%d,%s\n" % (s, i % 8, "ab"[i % 2]) for i, s in enumerate(iso)] + ["stranger,c8,a\n"]
    eight = _cfile(tmp_path, "Name,serotype,pair\n" + "".join(rows), "eight.csv")
    from scoary_amd import methods as m
    names, labels = m.read_categorical_file(eight, ",", iso)
    assert list(m._categorical_refusals(True, False, False, names, labels, exits=True)) == []
    assert len(m.categorical_classes(labels[0])) == 8


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import dist, methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    labels = [["a", "b", None]]
    for kw, text in ((dict(no_pairwise=False), "categorical traits need no_pairwise"),
                     (dict(collapse=True), "categorical traits exclude collapse"),
                     (dict(strata=[0, 0, 0]), "categorical traits exclude strata"),
                     (dict(no_pairwise=False, collapse=True), "categorical traits need no_pairwise")):
        with pytest.raises(ValueError, match=text):
            m.Categorical_results(None, ["x"], labels, **kw)
    with pytest.raises(ValueError, match="categorical trait sero has 9 classes, at most 8 are taken: merge rare classes"):
        m.Categorical_results(None, ["ok", "sero"], [["a", "b"] * 5, [str(i % 9) for i in range(10)]])
    monkeypatch.setattr(dist, "world_rank", lambda: (4, 1))
    with pytest.raises(ValueError, match="categorical traits need a single process"):
        m.Categorical_results(None, ["x"], labels)
    assert list(m.CATEGORICAL_TEXT) == ["no_pairwise", "collapse", "strata", "ranks", "classes"]
    assert [pair[0] for pair in m.CATEGORICAL_TEXT.values()][:4] == [NO_PAIRWISE, COLLAPSE, STRATA, RANKS]
    assert m.CATEGORICAL_TEXT["classes"][0] % ("sero", 9, 8) == CLASSES % ("sero", 9)


@pytest.mark.parametrize("delimiter", [",", ";"])
def test_reader_takes_labels_missing_spellings_and_the_tables_isolates(tmp_path, delimiter):
    from scoary_amd import methods as m
    strains = ["A", "B", "C", "D", "E", "F", "G"]
    rows = [["Name", "host", "sero group"],
            ["B", "pig", "O157"], ["A", "Pig", "NA"], ["zzz", "llama", "x"],            # an isolate the table has not
            ["C", "-", "1"], ["D", ".", " 1"], ["E", " ", "0"], ["F", "", "O157"]]       # G is absent
    path = _cfile(tmp_path, "".join(delimiter.join(r) + "\n" for r in rows))
    names, labels = m.read_categorical_file(path, delimiter, strains)
    assert names == ["host", "sero group"]
    assert labels == [["Pig", "pig", None, None, None, None, None], [None, "O157", "1", " 1", "0", "O157", None]]
    assert set(m.MISSING_TRAIT) == {"NA", "-", ".", " ", ""}                    # every spelling is in the rows above
    assert m.categorical_classes(labels[1]) == [" 1", "0", "1", "O157"]        # any string is a label, sorted as strings
    # -r applies through the table's strains
    names, labels = m.read_categorical_file(path, delimiter, ["B", "F"])
    assert labels == [["pig", None], ["O157", "O157"]]


def test_reader_refuses_a_malformed_file(tmp_path):
    from scoary_amd import methods as m
    for text, what in (("Name\nA\n", "contains at least one trait"), ("", "contains at least one trait"),
                       ("Name,x,x\nA,1,2\n", "names a trait more than once"),
                       ("Name,x\nA,1\nA,2\n", "names isolate A more than once"),
                       ("Name,x,y\nA,1\n", "has 2 cells in line 2, its header has 3")):
        with pytest.raises(SystemExit, match="The categorical traits file .* " + what + "|Please check that the "
                           "categorical traits file .* " + what):
            m.read_categorical_file(_cfile(tmp_path, text), ",", ["A"])


def test_most_enriched_class_compares_in_integers_and_prefers_the_first():
    from scoary_amd import methods as m
    assert m.most_enriched_class([1, 2, 0, 2], [2, 4, 0, 3]) == 3
    assert m.most_enriched_class([1, 2], [2, 4]) == 0                          # a tie goes to the first class
    assert m.most_enriched_class([0, 0, 5], [0, 7, 9]) == 2                    # an empty class is never the answer
    big = 3037000500                                                           # products past 2^63 stay exact
    assert m.most_enriched_class([big, big + 1], [big + 1, big + 2]) == 1


def test_the_feature_is_beside_the_pinned_tables_and_in_the_build():
    import __graft_entry__ as ge
    from scoary_amd import _abi, methods as m
    assert not any("chi2" in name.lower() for name, _k, _c in m.ALL_COLUMNS)
    assert not any(rule.flag == FLAG for rule in m.ALL_RULES)
    assert m.CATEGORICAL_COLUMNS == ("Number_with_gene", "Number_without_gene", "Carriers_by_class",
                                     "Most_enriched_class", "Chi2", "Chi2_df", "Cramers_V", "Chi2_p", "Bonferroni_p",
                                     "Benjamini_H_p")
    for name in ("scoary_categorical_max_classes", "scoary_categorical", "scoary_permute_categorical"):
        assert name in _abi.SIGNATURES
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert _abi.ABI_VERSION == 11 and "spec S20" in header and _abi.CATEGORICAL_MAX_CLASSES == 8
    assert any(s.endswith("scoary_categorical.hip") for s in ge.HIP_SRCS)
    # both translation units compile the one text of the chi-square tail
    csrc = os.path.dirname(ge.HIP_SRCS[0])
    for unit in ("scoary_cmh.hip", "scoary_categorical.hip"):
        with open(os.path.join(csrc, unit)) as f:
            text = f.read()
        assert '#include "scoary_chi2.hpp"' in text and "double chi2_tail(" not in text
    assert [r["name"] for r in ge.CATEGORICAL_RULES] == ["k_cat_observed", "k_cat_permute"]
    names = ["_ZN12_GLOBAL__N_114k_cat_observedEPK15HIP_vector_typeIjLj4EEl", "_ZN12_GLOBAL__N_113k_cat_permuteEPKjl"]
    ok = {n: {"VGPRs": 48, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0} for n in names}
    ge.check_kernel_resources(ok, ge.CATEGORICAL_RULES)
    for n in names:                                   # scratch or a spill in either kernel fails the build
        for field, what in (("ScratchSize", "scratch 8"), ("SGPRs Spill", "SGPR spills 8"), ("VGPRs Spill", "VGPR spills 8")):
            bad = {k: dict(v, **({field: 8} if k == n else {})) for k, v in ok.items()}
            with pytest.raises(RuntimeError, match=what):
                ge.check_kernel_resources(bad, ge.CATEGORICAL_RULES)
    with pytest.raises(RuntimeError, match="65 VGPRs > 64"):
        ge.check_kernel_resources({n: dict(v, VGPRs=65) for n, v in ok.items()}, ge.CATEGORICAL_RULES)
    every = (ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES +
             ge.CMH_HOMOG_RULES + ge.FISHER_CHAINS_RULES + ge.RANKSUM_RULES + ge.VANELTEREN_RULES + ge.RANK_WY_RULES +
             ge.RANK_SD_RULES + ge.RANK_SHIFT_RULES)
    for other in every:                               # and the new names are in no other family
        assert not any(other["name"] in n and not (other["exclude"] and other["exclude"] in n) for n in names)
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            ge.check_kernel_resources(json.load(f), ge.CATEGORICAL_RULES)
