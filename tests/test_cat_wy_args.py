"""--categorical-fwer: its refusals on the command line (they exit before the engine is touched) and in
Categorical_results / Gcmh_results, its column, and what the feature adds to the binding, the header and the build
(spec S22)."""
import os
import re

import numpy as np
import pytest

from args_cases import good_strata_file as _strata_file, run_refused as _run, strains as _strains

FLAG = "--categorical-fwer"
NEEDS_CATEGORICAL = ("Cannot use --categorical-fwer without --categorical. It is the family-wise p of the tests of the "
                     "categorical traits")
NEEDS_PERMUTE = ("Cannot use --categorical-fwer without --permute X, X >= 10. The family-wise p is counted over the "
                 "permutations of the labels")
ENTRY_POINTS = {"scoary_cat_wy_prepare": 11, "scoary_permute_cat_wy": 16, "scoary_permute_gcmh_wy": 14}
KERNELS = ["_ZN12_GLOBAL__N_116k_cat_wy_prepareEPKiS1_iiPdS2_S2_S2_",
           "_ZN12_GLOBAL__N_110k_cat_maxtEPKjliiPKsliPKiS5_PKmPKdS9_iiPiPdl",
           "_ZN12_GLOBAL__N_111k_gcmh_maxtEPKjliiPKsliPKdS5_PKiiiPiPdl"]


def _cfile(exampledir, tmp_path):
    path = os.path.join(str(tmp_path), "c.csv")
    with open(path, "w") as f:
        f.write("Name,host\n" + "".join("%s,%s\n" % (s, "ab"[i % 2]) for i, s in enumerate(_strains(exampledir))))
    return path


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.categorical_fwer is False
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", "--categorical", "c.csv",
                                         "-e", "100", FLAG])
    assert (args.categorical, args.categorical_fwer, args.permute) == ("c.csv", True, 100)


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    c = _cfile(exampledir, tmp_path)
    strata = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run(["--no_pairwise", FLAG]) == NEEDS_CATEGORICAL
    assert run(["--no_pairwise", "-e", "100", FLAG]) == NEEDS_CATEGORICAL
    assert run(["--no_pairwise", "--categorical", c, FLAG]) == NEEDS_PERMUTE
    assert run(["--no_pairwise", "--categorical", c, "--categorical-strata", strata, FLAG]) == NEEDS_PERMUTE
    # the rules of --categorical and of --categorical-strata come first
    assert run(["--categorical", c, "-e", "100", FLAG]).startswith("Cannot use --categorical without --no_pairwise")
    assert run(["--no_pairwise", "--categorical-strata", strata, "-e", "100", FLAG]).startswith(
        "Cannot use --categorical-strata without --categorical")
    # --permute 1 .. 9 is refused by --permute's own rule or by this one, never run
    assert isinstance(run(["--no_pairwise", "--categorical", c, "-e", "9", FLAG]), str)
    # the flag of the rank tests does not stand in for this one, nor this one for it
    assert run(["--no_pairwise", "--categorical", c, "-e", "100", "--quantitative-fwer"]).startswith(
        "Cannot use --quantitative-fwer without --quantitative")


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    labels = [["a", "b", None]]
    for perms in (0, 9):
        with pytest.raises(ValueError) as e:
            m.Categorical_results(None, ["x"], labels, permutations=perms, fwer=True)
        assert str(e.value) == NEEDS_PERMUTE
        with pytest.raises(SystemExit) as x:
            m.Categorical_results(None, ["x"], labels, permutations=perms, fwer=True, exits=True)
        assert str(x.value) == NEEDS_PERMUTE
        with pytest.raises(ValueError) as e:
            m.Gcmh_results(None, ["x"], labels, [0, 0, 1], permutations=perms, fwer=True)
        assert str(e.value) == NEEDS_PERMUTE
    # the rules of --categorical come first here too
    with pytest.raises(ValueError, match="categorical traits need no_pairwise"):
        m.Categorical_results(None, ["x"], labels, fwer=True, no_pairwise=False)
    with pytest.raises(ValueError, match="categorical traits exclude collapse"):
        m.Gcmh_results(None, ["x"], labels, [0, 0, 1], fwer=True, collapse=True)
    assert m.CAT_WY_TEXT == {"categorical": NEEDS_CATEGORICAL, "permute": NEEDS_PERMUTE}
    assert list(m._cat_wy_refusals(False, False, 0)) == []
    assert list(m._cat_wy_refusals(True, False, 0)) == [NEEDS_CATEGORICAL, NEEDS_PERMUTE]
    assert list(m._cat_wy_refusals(True, True, 9)) == [NEEDS_PERMUTE]
    assert list(m._cat_wy_refusals(True, True, 10)) == []


def test_the_binary_steps_tables_do_not_know_the_flag():
    from scoary_amd import methods as m
    assert not any(rule.flag == FLAG for rule in m.ALL_RULES) and not any(rule.flag == FLAG for rule in m.FLAG_RULES)
    assert not any("categorical" in name.lower() for name, _k, _c in m.ALL_COLUMNS)
    assert not any("categorical" in str(entry).lower() for entry in m.OPTIONAL_COLUMNS)
    # (the binary step has a column of that name of its own, for --permute-fwer: another file, another table)
    assert "Westfall_Young_p" not in m.CATEGORICAL_COLUMNS + m.GCMH_COLUMNS


def _results(store):
    common = dict(classes=["a", "b"], n=10, m=np.array([3, 4, 5, 0]), a=np.array([[1, 2], [3, 1], [2, 3], [0, 0]]),
                  p=np.array([0.04, 0.01, 0.04, 1.0]), testable=np.array([True, True, True, False]),
                  r=np.array([4, 0, 9, 20]), permutations=19)
    if store == "StoreCategoricalResults":
        return dict(common, nk=np.array([6, 4]), df=1, x2=np.array([4.2, 6.6, 4.2, 0.0]),
                    v=np.array([0.6, 0.8, 0.6, 0.0]))
    return dict(common, e=np.array([[1.5, 1.5], [2.0, 2.0], [2.5, 2.5], [0.0, 0.0]]), q=np.array([4.2, 6.6, 4.2, 0.0]),
                df=np.array([1, 1, 1, 0]))


@pytest.mark.parametrize("store, columns, suffix", (("StoreCategoricalResults", "CATEGORICAL_COLUMNS",
                                                     ".categorical.results.csv"),
                                                    ("StoreGcmhResults", "GCMH_COLUMNS", ".gcmh.results.csv")))
def test_the_column_and_the_store(tmp_path, monkeypatch, store, columns, suffix):
    from scoary_amd import methods as m

    class Table:
        ids, nugn, annotation, strains = ["a", "b_|_nb_|_ab", "c", "d"], ["na", "", "nc", "nd"], ["x", "", "y", "z"], []
    monkeypatch.setattr(m, "_as_table", lambda g: g)
    res = {"host": _results(store)}
    out = str(tmp_path) + os.sep
    (fname,) = getattr(m, store)(res, Table, None, out)
    without = open(fname).read().splitlines()
    assert without[0].endswith('"Empirical_p"')
    res["host"]["r_fwer"] = np.array([9, 1, 19, 19])
    (fname,) = getattr(m, store)(res, Table, None, out)
    assert fname == out + "host" + suffix
    lines = open(fname).read().splitlines()
    assert lines[0] == ",".join('"%s"' % c for c in m.ROARY_HEAD + list(getattr(m, columns)) +
                                ["Empirical_p", "Westfall_Young_p"])
    # one more cell at the end of every row, and nothing else changes
    assert [l.rsplit(",", 1)[0] for l in lines] == without
    assert [l.rsplit(",", 1)[1] for l in lines[1:]] == ['"0.1"', '"0.5"', '"1.0"']     # rows b, a, c
    # without permutations there is no column, whatever the dict holds
    del res["host"]["r"]
    (fname,) = getattr(m, store)(res, Table, None, out)
    assert "Westfall_Young_p" not in open(fname).read() and "Empirical_p" not in open(fname).read()


def test_the_entry_points_are_in_the_binding_the_header_and_the_build():
    import __graft_entry__ as ge
    from scoary_amd import _abi, engine
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert _abi.ABI_VERSION == 11 and "spec S22" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, code)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    # the entry points that were there keep their shapes
    assert len(_abi.SIGNATURES["scoary_permute_categorical"][1]) == 12
    assert len(_abi.SIGNATURES["scoary_permute_gcmh"][1]) == 12
    for name in ("categorical_wy_prepare", "categorical_westfall_young", "gcmh_westfall_young", "r_fwer_max"):
        assert callable(getattr(engine.AssociationEngine, name))
    assert any(s.endswith("scoary_cat_wy.hip") for s in ge.HIP_SRCS)
    # the three translation units compile the one text of the planes' walk, of the 128-bit product and of Q
    csrc = os.path.dirname(ge.HIP_SRCS[0])
    text = {}
    for unit in ("scoary_categorical.hip", "scoary_gcmh.hip", "scoary_cat_wy.hip", "scoary_cat_planes.hpp",
                 "scoary_gcmh_form.hpp"):
        with open(os.path.join(csrc, unit)) as f:
            text[unit] = f.read()
    for unit in ("scoary_categorical.hip", "scoary_gcmh.hip", "scoary_cat_wy.hip"):
        assert '#include "scoary_cat_planes.hpp"' in text[unit]
        assert "void cat_count(" not in text[unit] and "__int128 cat_mul(" not in text[unit]
        assert "double gcmh_q(" not in text[unit]
    for unit in ("scoary_gcmh.hip", "scoary_cat_wy.hip"):
        assert '#include "scoary_gcmh_form.hpp"' in text[unit]
    assert "__int128 cat_mul(" in text["scoary_cat_planes.hpp"] and "double gcmh_q(" in text["scoary_gcmh_form.hpp"]
    assert float(re.search(r"kCatWyBand = ([0-9.e-]+);", text["scoary_cat_wy.hip"]).group(1)) == 1e-9
    if os.path.exists(_abi.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_abi.LIB_PATH)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), name


def test_resource_rules():
    import __graft_entry__ as ge
    assert [r["name"] for r in ge.CAT_WY_RULES] == ["k_cat_wy_prepare", "k_cat_maxt", "k_gcmh_maxt"]
    assert ge.CAT_WY_RULES[1]["cap"] == ge.CAT_WY_RULES[2]["cap"] == (("VGPRs",), 128) == ge.GCMH_RULES[1]["cap"]
    assert all(r["scratch"] == 0 for r in ge.CAT_WY_RULES) and ge.CAT_WY_RULES[0]["sgpr_spills"] == 0
    ok = {n: {"VGPRs": 92, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0} for n in KERNELS}
    ge.check_kernel_resources(ok, ge.CAT_WY_RULES)
    for n in KERNELS:                                  # scratch or a spill in any of the three fails the build
        for field, what in (("ScratchSize", "scratch 64"), ("SGPRs Spill", "SGPR spills 64"),
                            ("VGPRs Spill", "VGPR spills 64")):
            bad = {k: dict(v, **({field: 64} if k == n else {})) for k, v in ok.items()}
            with pytest.raises(RuntimeError, match=what):
                ge.check_kernel_resources(bad, ge.CAT_WY_RULES)
    for n in KERNELS[1:]:
        with pytest.raises(RuntimeError, match="129 VGPRs > 128"):
            ge.check_kernel_resources({k: dict(v, VGPRs=129 if k == n else 92) for k, v in ok.items()}, ge.CAT_WY_RULES)
    with pytest.raises(RuntimeError, match="expected 1 k_gcmh_maxt instance, compiler reported 0"):
        ge.check_kernel_resources({n: ok[n] for n in KERNELS[:2]}, ge.CAT_WY_RULES)
    # the new kernels are in no other family: k_cat_permute, k_gcmh_permute and k_rank_maxt stay one kernel each
    every = (ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES +
             ge.CMH_HOMOG_RULES + ge.FISHER_CHAINS_RULES + ge.RANKSUM_RULES + ge.VANELTEREN_RULES + ge.RANK_WY_RULES +
             ge.RANK_SD_RULES + ge.RANK_SHIFT_RULES + ge.CATEGORICAL_RULES + ge.GCMH_RULES)
    for other in every:
        assert not any(other["name"] in n and not (other["exclude"] and other["exclude"] in n) for n in KERNELS), other
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            res = json.load(f)
        ge.check_kernel_resources(res, ge.CAT_WY_RULES)
        ge.check_kernel_resources(res, ge.CATEGORICAL_RULES)
        ge.check_kernel_resources(res, ge.GCMH_RULES)
