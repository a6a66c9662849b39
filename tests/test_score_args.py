"""--covariates FILE: the refusals on the command line (they exit before the engine is touched) and in Score_results
(the same rules as ValueErrors), the reader of the file, and what the feature adds beside the pinned tables, the
binding and the build."""
import os

import numpy as np
import pytest

from args_cases import run_refused as _run, strains as _strains

FLAG = "--covariates"
NO_PAIRWISE = ("Cannot use --covariates without --no_pairwise. The score test is a test of every gene; the "
               "covariates are its answer to population structure")
COLLAPSE = "Cannot use --covariates together with --collapse. The score test is a test of every gene of the table"
RANKS = "Cannot use --covariates under more than one rank: the test runs over all genes in a single process"
COLUMNS = ("Cannot use --covariates with the %d columns of %s: the score test adjusts for at most 8. Keep the leading "
           "axes of the structure and the confounders that matter")
ISOLATES = "The covariates file %s names none of the analysed isolates"


def _cfile(tmp_path, text, name="cov.csv"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def _good(exampledir, tmp_path, columns=2, name="cov.csv"):
    rows = ["%s,%s\n" % (s, ",".join("%d.5" % ((i * (k + 3)) % 7) for k in range(columns)))
            for i, s in enumerate(_strains(exampledir))]
    return _cfile(tmp_path, "Name," + ",".join("pc%d" % (k + 1) for k in range(columns)) + "\n" + "".join(rows), name)


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.covariates is None
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", FLAG, "c.csv"])
    assert args.covariates == "c.csv" and args.no_pairwise


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    from scoary_amd import dist
    c = _good(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run([FLAG, c]) == NO_PAIRWISE
    assert run([FLAG, c, "--collapse"]) == NO_PAIRWISE                          # in this order
    assert run(["--no_pairwise", FLAG, c, "--collapse"]) == COLLAPSE
    missing = os.path.join(str(tmp_path), "nowhere.csv")
    assert run(["--no_pairwise", FLAG, missing]) == "Could not find the covariates file: " + missing
    nine = _good(exampledir, tmp_path, columns=9, name="nine.csv")
    assert run(["--no_pairwise", FLAG, nine]) == COLUMNS % (9, nine)
    eight = _good(exampledir, tmp_path, columns=8, name="eight.csv")
    strangers = _cfile(tmp_path, "Name,pc1\nnobody,1.0\nno one,2.0\n", "strangers.csv")
    assert run(["--no_pairwise", FLAG, strangers]) == ISOLATES % strangers
    all_missing = _cfile(tmp_path, "Name,pc1\n" + "".join("%s,NA\n" % s for s in _strains(exampledir)), "na.csv")
    assert run(["--no_pairwise", FLAG, all_missing]) == ISOLATES % all_missing
    text = _cfile(tmp_path, "Name,pc1\n%s,high\n" % _strains(exampledir)[0], "text.csv")
    assert run(["--no_pairwise", FLAG, text]).startswith(
        "The covariates file %s has the cell 'high' for isolate %s, covariate pc1 (line 2): a cell is a finite number"
        % (text, _strains(exampledir)[0]))
    monkeypatch.setattr(dist, "world_rank", lambda: (2, 0))
    assert run(["--no_pairwise", FLAG, eight]) == RANKS


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import dist, methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    values, cov = np.array([[0.0, 1.0, np.nan]]), np.array([[0.5, 1.5, 2.5]])
    for kw, text in ((dict(no_pairwise=False), "covariates need no_pairwise"),
                     (dict(collapse=True), "covariates exclude collapse"),
                     (dict(no_pairwise=False, collapse=True), "covariates need no_pairwise")):
        with pytest.raises(ValueError, match=text):
            m.Score_results(None, ["x"], values, ["pc1"], cov, **kw)
    names = ["pc%d" % k for k in range(9)]
    with pytest.raises(ValueError, match="9 covariates .pc0, pc1, .*pc8., at most 8 are taken"):
        m.Score_results(None, ["x"], values, names, np.zeros((9, 3)))
    with pytest.raises(ValueError, match="the covariates .pc1. are missing for every isolate"):
        m.Score_results(None, ["x"], values, ["pc1"], np.full((1, 3), np.nan))
    monkeypatch.setattr(dist, "world_rank", lambda: (4, 1))
    with pytest.raises(ValueError, match="covariates need a single process"):
        m.Score_results(None, ["x"], values, ["pc1"], cov)
    assert list(m.SCORE_TEXT) == ["no_pairwise", "collapse", "ranks", "columns", "isolates"]
    assert [pair[0] for pair in m.SCORE_TEXT.values()][:3] == [NO_PAIRWISE, COLLAPSE, RANKS]
    assert m.SCORE_TEXT["columns"][0] % (9, "f.csv", 8) == COLUMNS % (9, "f.csv")
    assert m.SCORE_TEXT["isolates"][0] == ISOLATES


@pytest.mark.parametrize("delimiter", [",", ";"])
def test_reader_takes_numbers_missing_spellings_and_the_tables_isolates(tmp_path, delimiter):
    from scoary_amd import methods as m
    strains = ["A", "B", "C", "D", "E", "F", "G"]
    rows = [["Name", "pc1", "year"],
            ["B", "0.25", "2011"], ["A", "-1e-3", "NA"], ["zzz", "9", "9"],              # an isolate the table has not
            ["C", "-", "1999"], ["D", ".", " 2001"], ["E", " ", "0"], ["F", "", "2e3"]]   # G is absent
    path = _cfile(tmp_path, "".join(delimiter.join(r) + "\n" for r in rows))
    names, cov = m.read_covariates_file(path, delimiter, strains)
    assert names == ["pc1", "year"] and cov.shape == (2, 7) and cov.dtype == np.float64
    want = np.array([[-1e-3, 0.25] + [np.nan] * 5, [np.nan, 2011.0, 1999.0, 2001.0, 0.0, 2000.0, np.nan]])
    assert np.array_equal(cov, want, equal_nan=True)
    names, cov = m.read_covariates_file(path, delimiter, ["B", "F"])           # -r applies through the strains
    assert np.array_equal(cov, np.array([[0.25, np.nan], [2011.0, 2000.0]]), equal_nan=True)
    for text in ("inf", "nan", "1,5" if delimiter == ";" else "1;5"):
        bad = _cfile(tmp_path, delimiter.join(["Name", "pc1"]) + "\n" + delimiter.join(["A", text]) + "\n", "bad.csv")
        with pytest.raises(SystemExit, match="a cell is a finite number or one of"):
            m.read_covariates_file(bad, delimiter, strains)


def test_binary_trait_values_follow_the_traits_file():
    from scoary_amd import methods as m
    names, values = m.binary_trait_values({"res": {"A": "1", "B": "0"}, "vir": {"C": "1", "A": "0", "B": "1"}},
                                          ["A", "B", "C"])
    assert names == ["res", "vir"]
    assert np.array_equal(values, np.array([[1.0, 0.0, np.nan], [0.0, 1.0, 1.0]]), equal_nan=True)


def test_the_feature_is_beside_the_pinned_tables_and_in_the_build():
    import re
    import __graft_entry__ as ge
    from scoary_amd import _abi, engine, methods as m
    assert not any(name in ("Beta", "Std_err", "Score_p", "Linear_p") for name, _k, _c in m.ALL_COLUMNS)
    assert not any(rule.flag == FLAG for rule in m.ALL_RULES)
    assert m.LOGISTIC_COLUMNS == ("Number_with_gene", "Number_without_gene", "Beta", "Std_err", "Odds_ratio",
                                  "Score_chi2", "Score_p", "Bonferroni_p", "Benjamini_H_p")
    assert m.LINEAR_COLUMNS == ("Number_with_gene", "Number_without_gene", "Beta", "Std_err", "T_stat", "Linear_p",
                                "Bonferroni_p", "Benjamini_H_p")
    assert _abi.ABI_VERSION == 11 and _abi.SCORE_MAX_COVARIATES == 8 == engine.SCORE_MAX_COVARIATES
    # header, table and library name the same entry points with the same number of arguments
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert "spec S24" in header
    for name in ("scoary_score_max_covariates", "scoary_score"):
        assert name in _abi.SIGNATURES
        (proto,) = re.findall(r"\n(?:int|int64_t) %s\(([^;]*)\);" % name, header)
        count = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert count == len(_abi.SIGNATURES[name][1]), name
    if os.path.exists(_abi.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_abi.LIB_PATH)
        assert lib.scoary_score_max_covariates() == 8 and lib.scoary_abi_version() == 11
        assert hasattr(lib, "scoary_score")
    assert any(s.endswith("scoary_score.hip") for s in ge.HIP_SRCS)
    csrc = os.path.dirname(ge.HIP_SRCS[0])
    with open(os.path.join(csrc, "scoary_score.hip")) as f:
        text = f.read()
    assert '#include "scoary_chi2.hpp"' in text and '#include "scoary_ttail.hpp"' in text
    assert "double chi2_tail(" not in text and os.path.exists(os.path.join(csrc, "scoary_ttail.hpp"))
    assert [r["name"] for r in ge.SCORE_RULES] == ["k_score_observed"] and ge.SCORE_RULES[0]["count"] == 9
    names = ["_ZN12_GLOBAL__N_116k_score_observedILi%dEEEvPK15HIP_vector_typeIjLj4EEliiii" % q for q in range(1, 10)]
    ok = {n: {"VGPRs": 100, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0} for n in names}
    ge.check_kernel_resources(ok, ge.SCORE_RULES)
    for field, what in (("ScratchSize", "scratch 8"), ("SGPRs Spill", "SGPR spills 8"), ("VGPRs Spill", "VGPR spills 8")):
        bad = {k: dict(v, **({field: 8} if k == names[4] else {})) for k, v in ok.items()}
        with pytest.raises(RuntimeError, match=what):
            ge.check_kernel_resources(bad, ge.SCORE_RULES)
    cap = ge.SCORE_RULES[0]["cap"][1]
    with pytest.raises(RuntimeError, match="%d VGPRs > %d" % (cap + 1, cap)):
        ge.check_kernel_resources({n: dict(v, VGPRs=cap + 1) for n, v in ok.items()}, ge.SCORE_RULES)
    with pytest.raises(RuntimeError, match="expected 9 k_score_observed instances, compiler reported 8"):
        ge.check_kernel_resources({n: ok[n] for n in names[:8]}, ge.SCORE_RULES)
    every = (ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES +
             ge.CMH_HOMOG_RULES + ge.FISHER_CHAINS_RULES + ge.RANKSUM_RULES + ge.VANELTEREN_RULES + ge.RANK_WY_RULES +
             ge.RANK_SD_RULES + ge.RANK_SHIFT_RULES + ge.CATEGORICAL_RULES + ge.GCMH_RULES + ge.CAT_WY_RULES +
             ge.CAT_SD_RULES)
    for other in every:                               # and the new name is in no other family
        assert not any(other["name"] in n and not (other["exclude"] and other["exclude"] in n) for n in names)
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            ge.check_kernel_resources(json.load(f), ge.SCORE_RULES)
