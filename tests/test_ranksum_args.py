"""--quantitative FILE: the four refusals on the command line (they exit before the engine is touched) and in
Ranksum_results (the same rules as ValueErrors), the reader of the file, and what the feature adds beside the pinned
tables, the binding and the build."""
import os

import numpy as np
import pytest

from args_cases import good_strata_file as _strata_file, run_refused as _run

FLAG = "--quantitative"
NO_PAIRWISE = ("Cannot use --quantitative without --no_pairwise. The rank-sum test is a population structure-naive "
               "test of every gene")
COLLAPSE = ("Cannot use --quantitative together with --collapse. The rank-sum test is a test of every gene of the "
            "table")
STRATA = ("Cannot use --quantitative together with --permute-strata. The values are shuffled over all isolates with a "
          "value; a shuffle within strata is not implemented")
RANKS = "Cannot use --quantitative under more than one rank: the test runs over all genes in a single process"


def _qfile(tmp_path, text="Name,mic\nA,1.5\n", name="q.csv"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def test_flag_is_off_by_default_and_keeps_the_traits_file_required():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.quantitative is None
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", FLAG, "q.csv", "-e", "50"])
    assert args.quantitative == "q.csv" and args.permute == 50 and args.no_pairwise
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", FLAG, "q.csv"])
    assert args.traits is None
    with pytest.raises(SystemExit, match="The following arguments are required: -t/--traits, -g/--genes"):
        m._validate(args, _cut)


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    from scoary_amd import dist
    q = _qfile(tmp_path)
    strata = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run([FLAG, q]) == NO_PAIRWISE
    assert run([FLAG, q, "--collapse"]) == NO_PAIRWISE                          # in this order
    assert run(["--no_pairwise", FLAG, q, "--collapse"]) == COLLAPSE
    assert run(["--no_pairwise", FLAG, q, "-e", "100", "--permute-strata", strata]) == STRATA
    assert run(["--no_pairwise", FLAG, q, "--collapse", "-e", "100", "--permute-strata", strata]) == COLLAPSE
    missing = os.path.join(str(tmp_path), "nowhere.csv")
    assert run(["--no_pairwise", FLAG, missing]) == "Could not find the quantitative traits file: " + missing
    assert run(["--no_pairwise", FLAG, q, "-e", "5"]) == \
        "The absolute minimum number of permutations is 10 (or 0 to deactivate)"
    monkeypatch.setattr(dist, "world_rank", lambda: (2, 0))
    assert run(["--no_pairwise", FLAG, q]) == RANKS


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import dist, methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    vals = np.zeros((1, 3))
    for kw, text in ((dict(no_pairwise=False), "quantitative traits need no_pairwise"),
                     (dict(collapse=True), "quantitative traits exclude collapse"),
                     (dict(strata=np.zeros(3, dtype=np.int64)), "quantitative traits exclude strata"),
                     (dict(no_pairwise=False, collapse=True), "quantitative traits need no_pairwise")):
        with pytest.raises(ValueError, match=text):
            m.Ranksum_results(None, ["x"], vals, **kw)
    monkeypatch.setattr(dist, "world_rank", lambda: (4, 1))
    with pytest.raises(ValueError, match="quantitative traits need a single process"):
        m.Ranksum_results(None, ["x"], vals)
    assert [pair[0] for pair in m.RANKSUM_TEXT.values()] == [NO_PAIRWISE, COLLAPSE, STRATA, RANKS]


@pytest.mark.parametrize("delimiter", [",", ";"])
def test_reader_takes_numbers_missing_spellings_and_the_tables_isolates(tmp_path, delimiter):
    from scoary_amd import methods as m
    strains = ["A", "B", "C", "D", "E", "F", "G"]
    rows = [["Name", "mic", "growth rate"],
            ["B", "0.25", "1e-3"], ["A", "4", "NA"], ["zzz", "17", "18"],           # an isolate the table has not
            ["C", "-", "-2.5"], ["D", ".", " 3 "], ["E", " ", "7"], ["F", "", "+.5"]]       # G is absent
    path = _qfile(tmp_path, "".join(delimiter.join(r) + "\n" for r in rows))
    names, vals = m.read_quantitative_file(path, delimiter, strains)
    nan = np.nan
    assert names == ["mic", "growth rate"] and vals.dtype == np.float64 and vals.shape == (2, 7)
    want = np.array([[4.0, 0.25, nan, nan, nan, nan, nan], [nan, 1e-3, -2.5, 3.0, 7.0, 0.5, nan]])
    assert np.array_equal(vals, want, equal_nan=True)
    assert set(m.MISSING_TRAIT) == {"NA", "-", ".", " ", ""}                    # every spelling is in the rows above
    # -r applies through the table's strains
    names, vals = m.read_quantitative_file(path, delimiter, ["B", "F"])
    assert np.array_equal(vals, np.array([[0.25, nan], [1e-3, 0.5]]), equal_nan=True)


@pytest.mark.parametrize("cell", ["high", "nan", "inf", "-Infinity", "1,5", "0x10", "NaN"])
def test_reader_refuses_a_cell_that_is_no_finite_number(tmp_path, cell):
    from scoary_amd import methods as m
    path = _qfile(tmp_path, "Name;mic\nA;1\nB;%s\n" % cell)
    with pytest.raises(SystemExit, match="has the cell %r for isolate B, trait mic" % cell):
        m.read_quantitative_file(path, ";", ["A", "B"])
    # (an isolate the analysis does not hold is not read at all)
    names, vals = m.read_quantitative_file(path, ";", ["A"])
    assert vals.tolist() == [[1.0]]


def test_reader_refuses_a_malformed_file(tmp_path):
    from scoary_amd import methods as m
    for text, what in (("Name\nA\n", "contains at least one trait"), ("", "contains at least one trait"),
                       ("Name,x,x\nA,1,2\n", "names a trait more than once"),
                       ("Name,x\nA,1\nA,2\n", "names isolate A more than once"),
                       ("Name,x,y\nA,1\n", "has 2 cells in line 2, its header has 3")):
        with pytest.raises(SystemExit, match=what):
            m.read_quantitative_file(_qfile(tmp_path, text), ",", ["A"])


def test_the_feature_is_beside_the_pinned_tables_and_in_the_build():
    import __graft_entry__ as ge
    from scoary_amd import _abi, methods as m
    assert not any("rank" in name.lower() for name, _k, _c in m.ALL_COLUMNS)
    assert not any(rule.flag == FLAG for rule in m.ALL_RULES)
    assert m.RANKSUM_COLUMNS == ("Number_with_gene", "Number_without_gene", "Rank_sum_AUC", "Rank_sum_p",
                                 "Bonferroni_p", "Benjamini_H_p")
    for name in ("scoary_ranksum_max_isolates", "scoary_ranksum", "scoary_ranksum_perm_generate",
                 "scoary_ranksum_bfrag_bytes", "scoary_ranksum_perm_generate_bfrag", "scoary_permute_ranksum"):
        assert name in _abi.SIGNATURES
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert _abi.ABI_VERSION == 11 and "spec S15" in header
    assert any(s.endswith("scoary_ranksum.hip") for s in ge.HIP_SRCS)
    assert [r["name"] for r in ge.RANKSUM_RULES] == ["k_ranksumE", "k_ranksum_labels", "k_permute_ranksum"]
    names = ["_ZN12_GLOBAL__N_19k_ranksumEPKj", "_ZN12_GLOBAL__N_116k_ranksum_labelsEPKs",
             "_ZN12_GLOBAL__N_117k_permute_ranksumEPKh"]
    ok = {n: {"VGPRs": 100, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0} for n in names}
    ge.check_kernel_resources(ok, ge.RANKSUM_RULES)
    for n in names:                                   # scratch in any kernel of the file fails the build
        bad = {k: dict(v, ScratchSize=8 if k == n else 0) for k, v in ok.items()}
        with pytest.raises(RuntimeError, match="scratch 8"):
            ge.check_kernel_resources(bad, ge.RANKSUM_RULES)
    for other in ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES:       # and it is in no other family
        assert not any(other["name"] in n and not (other["exclude"] and other["exclude"] in n) for n in names)
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            ge.check_kernel_resources(json.load(f), ge.RANKSUM_RULES)
