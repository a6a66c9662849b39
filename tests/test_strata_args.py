"""--permute-strata: the argument checks (host only -- they exit before the engine is touched; the declarations of
the stratified entry points: test_host_logic.py)."""
import os

import pytest

from args_cases import good_rows, run_refused as _run, strains as _strains, strata_file


def _strata_file(tmp_path, rows, name="strata.csv", header="Isolate,Stratum,Note"):
    return strata_file(tmp_path, rows, name, header)                        # (a third column: it is ignored)


def _good_rows(exampledir):
    return good_rows(exampledir, "x")


def test_refused_without_no_pairwise_or_permutations(exampledir, tmp_path, monkeypatch):
    path = _strata_file(tmp_path, _good_rows(exampledir))
    for argv, message in (
            (["--permute-strata", path, "-e", "100"], "Cannot use --permute-strata without --no_pairwise"),
            (["--permute-strata", path, "--no_pairwise"], "Cannot use --permute-strata without performing permutations"),
            (["--permute-strata", path, "--no_pairwise", "-e", "5"],
             "Cannot use --permute-strata without performing permutations")):
        code = _run(argv, exampledir, tmp_path, monkeypatch)
        assert isinstance(code, str) and code.startswith(message), code


def test_refused_file_problems(exampledir, tmp_path, monkeypatch):
    base = ["--no_pairwise", "-e", "100", "--permute-strata"]
    good = _good_rows(exampledir)
    code = _run(base + [os.path.join(str(tmp_path), "nowhere.csv")], exampledir, tmp_path, monkeypatch)
    assert isinstance(code, str) and code.startswith("Could not find the strata file"), code
    code = _run(base + [_strata_file(tmp_path, good[:-1], "absent.csv")], exampledir, tmp_path, monkeypatch)
    assert isinstance(code, str) and "does not name a stratum for 1 of the analysed isolates" in code \
        and good[-1][0] in code, code
    empty = list(good)
    empty[4] = (empty[4][0], "", "x")
    code = _run(base + [_strata_file(tmp_path, empty, "empty.csv")], exampledir, tmp_path, monkeypatch)
    assert isinstance(code, str) and "empty stratum label for isolate %s" % empty[4][0] in code, code
    code = _run(base + [_strata_file(tmp_path, good + [good[2]], "twice.csv")], exampledir, tmp_path, monkeypatch)
    assert isinstance(code, str) and "names isolate %s more than once" % good[2][0] in code, code


def test_refused_above_the_generator_limits(exampledir, tmp_path, monkeypatch):
    from scoary_amd import _abi
    base = ["--no_pairwise", "-e", "100", "--permute-strata"]
    own = [(s, "own%d" % i) for i, s in enumerate(_strains(exampledir))]
    path = _strata_file(tmp_path, own, "own.csv")
    monkeypatch.setattr(_abi, "PERM_MAX_STRATA", len(own) - 1)
    code = _run(base + [path], exampledir, tmp_path, monkeypatch)
    assert isinstance(code, str) and "--permute-strata takes at most %d" % (len(own) - 1) in code, code
    monkeypatch.setattr(_abi, "PERM_MAX_STRATA", 1024)
    monkeypatch.setattr(_abi, "PERM_STRATA_MAX_ISOLATES", len(own) - 1)
    code = _run(base + [path], exampledir, tmp_path, monkeypatch)
    assert isinstance(code, str) and code.startswith("--permute-strata takes at most %d isolates" % (len(own) - 1)), code


def test_isolates_outside_the_analysis_are_ignored_and_labels_numbered_by_first_appearance(exampledir, tmp_path):
    from scoary_amd import methods as m
    strains = _strains(exampledir)
    rows = [("not_analysed", "zzz")] + [(s, ("b", "a", "c")[i % 3]) for i, s in reversed(list(enumerate(strains)))]
    smap = m.read_strata_file(_strata_file(tmp_path, rows, header="name;with,odd header"))
    idx, labels = m.strata_indices(smap, strains)
    assert labels == ["b", "a", "c"] and idx.tolist() == [i % 3 for i in range(len(strains))]
    idx, labels = m.strata_indices(smap, strains[1:3])              # after -r: numbered along what is analysed
    assert labels == ["a", "c"] and idx.tolist() == [0, 1]
    # another delimiter
    path = os.path.join(str(tmp_path), "semi.csv")
    with open(path, "w") as f:
        f.write("Isolate;Stratum\n" + "".join("%s;ST %d\n" % (s, i // 10) for i, s in enumerate(strains)))
    assert m.read_strata_file(path, ";")[strains[11]] == "ST 1"


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.permute_strata is None
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--permute-strata", "s.csv"])
    assert args.permute_strata == "s.csv"


def test_setup_results_refuses_strata_without_permutations():
    from scoary_amd import methods as m
    with pytest.raises(ValueError):
        m.Setup_results({}, {}, False, permutations=0, strata=[0, 1])
