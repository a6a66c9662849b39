"""--quantitative-strata FILE: its refusals on the command line (they exit before the engine is touched) and in
VanElteren_results, its columns, and what the feature adds to the binding, the header and the build."""
import os
import re

import numpy as np
import pytest

from args_cases import good_strata_file as _strata_file, run_refused as _run, strains as _strains, strata_file

FLAG = "--quantitative-strata"
NEEDS_QUANTITATIVE = ("Cannot use --quantitative-strata without --quantitative. Its strata are those of the van "
                      "Elteren test of the measured traits")
ENTRY_POINTS = ("scoary_vanelteren", "scoary_vanelteren_perm_generate", "scoary_vanelteren_perm_generate_bfrag")


def _qfile(tmp_path, text="Name,mic\nA,1.5\n", name="q.csv"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.quantitative_strata is None
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", "--quantitative", "q.csv",
                                         FLAG, "s.csv"])
    assert (args.quantitative, args.quantitative_strata, args.permute_strata) == ("q.csv", "s.csv", None)


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    from scoary_amd import _abi
    q = _qfile(tmp_path)
    strata = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run(["--no_pairwise", FLAG, strata]) == NEEDS_QUANTITATIVE
    assert run([FLAG, strata]) == NEEDS_QUANTITATIVE
    missing = os.path.join(str(tmp_path), "nowhere.csv")
    assert run(["--no_pairwise", "--quantitative", q, FLAG, missing]) == \
        "Could not find the strata file of --quantitative-strata: " + missing
    # the rules of --quantitative come first, and its refusal of --permute-strata stands
    assert run(["--quantitative", q, FLAG, strata]).startswith("Cannot use --quantitative without --no_pairwise")
    assert run(["--no_pairwise", "--quantitative", q, FLAG, strata, "-e", "100", "--permute-strata", strata]) \
        .startswith("Cannot use --quantitative together with --permute-strata")
    own = [(s, "own%d" % i) for i, s in enumerate(_strains(exampledir))]
    path = strata_file(tmp_path, own, "own.csv")
    monkeypatch.setattr(_abi, "PERM_MAX_STRATA", len(own) - 1)
    assert run(["--no_pairwise", "--quantitative", q, FLAG, path]) == \
        "The strata file %s names %d strata for the analysed isolates; --quantitative-strata takes at most %d" \
        % (path, len(own), len(own) - 1)
    monkeypatch.setattr(_abi, "PERM_MAX_STRATA", 1024)
    # an isolate of the analysis without a stratum, an empty label: the strata file reader's own exits
    assert "does not name a stratum for 1 of the analysed isolates" in \
        run(["--no_pairwise", "--quantitative", q, FLAG, strata_file(tmp_path, own[1:], "short.csv")])


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    vals, st = np.zeros((1, 3)), np.zeros(3, dtype=np.int64)
    for kw, text in ((dict(no_pairwise=False), "quantitative traits need no_pairwise"),
                     (dict(collapse=True), "quantitative traits exclude collapse")):
        with pytest.raises(ValueError, match=text):
            m.VanElteren_results(None, ["x"], vals, st, **kw)
    assert list(m.VANELTEREN_TEXT) == ["quantitative", "file", "strata"]
    assert m.VANELTEREN_TEXT["quantitative"] == NEEDS_QUANTITATIVE


def test_columns_and_the_store(tmp_path, monkeypatch):
    from scoary_amd import methods as m
    assert m.VANELTEREN_COLUMNS == ("Number_with_gene", "Number_without_gene", "Van_Elteren_AUC", "Van_Elteren_p",
                                    "Bonferroni_p", "Benjamini_H_p")
    assert m.RANKSUM_COLUMNS[2:4] == ("Rank_sum_AUC", "Rank_sum_p")
    assert not any("elteren" in name.lower() for name, _k, _c in m.ALL_COLUMNS)
    assert not any(rule.flag == FLAG for rule in m.ALL_RULES)

    class Table:
        ids, nugn, annotation, strains = ["a", "b_|_nb_|_ab", "c", "d"], ["na", "", "nc", "nd"], ["x", "", "y", "z"], []
    monkeypatch.setattr(m, "_as_table", lambda g: g)
    res = {"mic": dict(n=10, m=np.array([3, 4, 5, 0]), auc=np.array([0.75, 0.25, 0.5, 0.5]),
                       p=np.array([0.04, 0.01, 0.04, 1.0]), testable=np.array([True, True, True, False]),
                       r=np.array([4, 0, 9, 20]), permutations=19)}
    out = str(tmp_path) + os.sep
    (fname,) = m.StoreVanElterenResults(res, Table, None, out)
    assert fname == out + "mic.vanelteren.results.csv"
    lines = open(fname).read().splitlines()
    assert lines[0] == ",".join('"%s"' % c for c in m.ROARY_HEAD + list(m.VANELTEREN_COLUMNS) + ["Empirical_p"])
    assert [l.split(",")[0] for l in lines[1:]] == ['"b"', '"a"', '"c"']   # ascending p, ties in file order
    assert lines[1] == '"b","nb","ab","4","6","0.25","0.01","0.03","0.03","0.05"'
    assert lines[2].split(",")[3:] == ['"3"', '"7"', '"0.75"', '"0.04"', '"0.12"', '"0.04"', '"0.25"']
    (fname,) = m.StoreVanElterenResults(res, Table, 1, out, time="_t", delimiter=";")
    assert fname.endswith("mic_t.vanelteren.results.csv") and len(open(fname).read().splitlines()) == 2


def test_the_entry_points_are_in_the_binding_the_header_and_the_build():
    import __graft_entry__ as ge
    from scoary_amd import _abi
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert _abi.ABI_VERSION == 11 and "spec S16" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in _abi.SIGNATURES
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, code)
        assert decl and len(decl.group(1).split(",")) == len(_abi.SIGNATURES[name][1]), name
    assert len(_abi.SIGNATURES["scoary_vanelteren"][1]) == 19
    assert _abi.SIGNATURES["scoary_vanelteren_perm_generate"] == _abi.SIGNATURES["scoary_vanelteren_perm_generate_bfrag"]
    assert any(s.endswith("scoary_vanelteren.hip") for s in ge.HIP_SRCS)
    assert any(s.endswith("scoary_ranksum.hip") for s in ge.HIP_SRCS)


def test_resource_rules():
    import __graft_entry__ as ge
    assert [r["name"] for r in ge.VANELTEREN_RULES] == ["k_vanelterenE", "k_vanelteren_labels"]
    assert ge.VANELTEREN_RULES[1]["cap"] == (("VGPRs",), 128) == ge.RANKSUM_RULES[1]["cap"]
    names = ["_ZN12_GLOBAL__N_112k_vanelterenEPK15HIP_vector_typeIjLj4EEl",
             "_ZN12_GLOBAL__N_119k_vanelteren_labelsEPKsPKjPKt"]
    ok = {n: {"VGPRs": 100, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0} for n in names}
    ge.check_kernel_resources(ok, ge.VANELTEREN_RULES)
    for n in names:                                   # scratch or a spill in either kernel fails the build
        for field, text in (("ScratchSize", "scratch 8"), ("VGPRs Spill", "VGPR spills 8"),
                            ("SGPRs Spill", "SGPR spills 8")):
            bad = {k: dict(v, **{field: 8 if k == n else 0}) for k, v in ok.items()}
            with pytest.raises(RuntimeError, match=text):
                ge.check_kernel_resources(bad, ge.VANELTEREN_RULES)
    with pytest.raises(RuntimeError, match="129 VGPRs > 128"):
        ge.check_kernel_resources({k: dict(v, VGPRs=129) for k, v in ok.items()}, ge.VANELTEREN_RULES)
    with pytest.raises(RuntimeError, match="expected 1 k_vanelteren_labels instance, compiler reported 0"):
        ge.check_kernel_resources({names[0]: ok[names[0]]}, ge.VANELTEREN_RULES)
    # no kernel of the file is in another family, and no other family's kernel is in this one
    every = (ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES + ge.RANKSUM_RULES + ge.CMH_EXACT_RULES +
             ge.CMH_EXACT_ODDS_RULES + ge.CMH_HOMOG_RULES + ge.FISHER_CHAINS_RULES)
    for other in every:
        assert not any(other["name"] in n and not (other["exclude"] and other["exclude"] in n) for n in names), other
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            res = json.load(f)
        ge.check_kernel_resources(res, ge.VANELTEREN_RULES)
        ge.check_kernel_resources(res, ge.RANKSUM_RULES)
        for rule in ge.VANELTEREN_RULES:
            (hit,) = [k for k in res if rule["name"] in k]
            assert not any(o["name"] in hit for o in every)
