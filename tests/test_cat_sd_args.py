"""--categorical-fwer-stepdown: its refusals on the command line (they exit before the engine is touched) and in
Categorical_results / Gcmh_results, its column, and what the feature adds to the binding, the header and the build
(spec S23)."""
import os
import re

import numpy as np
import pytest

from args_cases import good_strata_file as _strata_file, run_refused as _run, strains as _strains

FLAG = "--categorical-fwer-stepdown"
NEEDS_CATEGORICAL = ("Cannot use --categorical-fwer-stepdown without --categorical. It is the step-down family-wise p "
                     "of the tests of the categorical traits")
NEEDS_PERMUTE = ("Cannot use --categorical-fwer-stepdown without --permute X, X >= 10. The family-wise p is counted "
                 "over the permutations of the labels")
ENTRY_POINTS = {"scoary_cat_stepdown_scratch_bytes": 6, "scoary_cat_stepdown_gather": 11,
                "scoary_gcmh_stepdown_gather": 10, "scoary_permute_cat_stepdown": 16,
                "scoary_permute_gcmh_stepdown": 14}
KERNELS = ["_ZN12_GLOBAL__N_115k_cat_sd_gatherEPK15HIP_vector_typeIjLj4EElPKiiliPKmiPKdS9_PS1_PmPdSC_",
           "_ZN12_GLOBAL__N_115k_cat_sd_suffixEPdilllS0_l",
           "_ZN12_GLOBAL__N_112k_cat_sd_maxEPKjliiiPKsliPKiPKdS5_PKmS7_iiPiPd",
           "_ZN12_GLOBAL__N_114k_cat_sd_countEPKjliiiPKsliPKiPKdS7_S5_S7_iiPiPd",
           "_ZN12_GLOBAL__N_113k_gcmh_sd_maxEPKjliiiPKsliPKdS5_PKiiiPiPd",
           "_ZN12_GLOBAL__N_115k_gcmh_sd_countEPKjliiiPKsliPKdS5_PKiiiPiPd"]
HOT = KERNELS[2:]


def _cfile(exampledir, tmp_path):
    path = os.path.join(str(tmp_path), "c.csv")
    with open(path, "w") as f:
        f.write("Name,host\n" + "".join("%s,%s\n" % (s, "ab"[i % 2]) for i, s in enumerate(_strains(exampledir))))
    return path


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.categorical_fwer_stepdown is False
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", "--categorical", "c.csv",
                                         "-e", "100", FLAG])
    assert (args.categorical, args.categorical_fwer_stepdown, args.categorical_fwer, args.permute) == \
        ("c.csv", True, False, 100)


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    c = _cfile(exampledir, tmp_path)
    strata = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run(["--no_pairwise", FLAG]) == NEEDS_CATEGORICAL
    assert run(["--no_pairwise", "-e", "100", FLAG]) == NEEDS_CATEGORICAL
    assert run(["--no_pairwise", "--categorical", c, FLAG]) == NEEDS_PERMUTE
    assert run(["--no_pairwise", "--categorical", c, "--categorical-strata", strata, FLAG]) == NEEDS_PERMUTE
    # the rules of --categorical, of --categorical-strata and of --categorical-fwer come first
    assert run(["--categorical", c, "-e", "100", FLAG]).startswith("Cannot use --categorical without --no_pairwise")
    assert run(["--no_pairwise", "--categorical-strata", strata, "-e", "100", FLAG]).startswith(
        "Cannot use --categorical-strata without --categorical")
    assert run(["--no_pairwise", "--categorical-fwer", FLAG]).startswith(
        "Cannot use --categorical-fwer without --categorical.")
    assert run(["--no_pairwise", "--categorical", c, "--categorical-fwer", FLAG]).startswith(
        "Cannot use --categorical-fwer without --permute")
    # --permute 1 .. 9 is refused by --permute's own rule or by this one, never run
    assert isinstance(run(["--no_pairwise", "--categorical", c, "-e", "9", FLAG]), str)
    # the flag of the rank tests does not stand in for this one, nor this one for it
    assert run(["--no_pairwise", "--categorical", c, "-e", "100", "--quantitative-fwer-stepdown"]).startswith(
        "Cannot use --quantitative-fwer-stepdown without --quantitative")


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    labels = [["a", "b", None]]
    for perms in (0, 9):
        with pytest.raises(ValueError) as e:
            m.Categorical_results(None, ["x"], labels, permutations=perms, stepdown=True)
        assert str(e.value) == NEEDS_PERMUTE
        with pytest.raises(SystemExit) as x:
            m.Categorical_results(None, ["x"], labels, permutations=perms, stepdown=True, exits=True)
        assert str(x.value) == NEEDS_PERMUTE
        with pytest.raises(ValueError) as e:
            m.Gcmh_results(None, ["x"], labels, [0, 0, 1], permutations=perms, stepdown=True)
        assert str(e.value) == NEEDS_PERMUTE
        # --categorical-fwer's rule comes first
        with pytest.raises(ValueError) as e:
            m.Categorical_results(None, ["x"], labels, permutations=perms, fwer=True, stepdown=True)
        assert str(e.value) == m.CAT_WY_TEXT["permute"]
    # the rules of --categorical come first here too
    with pytest.raises(ValueError, match="categorical traits need no_pairwise"):
        m.Categorical_results(None, ["x"], labels, stepdown=True, no_pairwise=False)
    with pytest.raises(ValueError, match="categorical traits exclude collapse"):
        m.Gcmh_results(None, ["x"], labels, [0, 0, 1], stepdown=True, collapse=True)
    assert m.CAT_SD_TEXT == {"categorical": NEEDS_CATEGORICAL, "permute": NEEDS_PERMUTE}
    assert list(m._cat_sd_refusals(False, False, 0)) == []
    assert list(m._cat_sd_refusals(True, False, 0)) == [NEEDS_CATEGORICAL, NEEDS_PERMUTE]
    assert list(m._cat_sd_refusals(True, True, 9)) == [NEEDS_PERMUTE]
    assert list(m._cat_sd_refusals(True, True, 10)) == []
    # worded after the rank tests' two messages, with the categorical flag names
    for key, mine in m.CAT_SD_TEXT.items():
        theirs = m.RANK_SD_TEXT[key.replace("categorical", "quantitative")].replace("--quantitative", "--categorical")
        assert mine.split(". ")[0] == theirs.split(". ")[0], key


def test_the_binary_steps_tables_do_not_know_the_flag():
    from scoary_amd import methods as m
    assert not any(rule.flag == FLAG for rule in m.ALL_RULES) and not any(rule.flag == FLAG for rule in m.FLAG_RULES)
    assert not any("categorical" in name.lower() for name, _k, _c in m.ALL_COLUMNS)
    assert not any("categorical" in str(entry).lower() for entry in m.OPTIONAL_COLUMNS)
    assert not any(key == "r_sd" for _name, key, _c in m.ALL_COLUMNS)
    assert "Westfall_Young_stepdown_p" not in m.CATEGORICAL_COLUMNS + m.GCMH_COLUMNS
    assert m.PERMUTATION_COLUMNS[2] == ("Westfall_Young_stepdown_p", "r_sd")


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
    # a result that carries r_sd gets the column where the store is asked for it (the flag), and only there
    res["host"]["r_sd"] = np.array([9, 1, 14, 19])
    (fname,) = getattr(m, store)(res, Table, None, out)
    assert open(fname).read().splitlines() == without
    # the flag alone: r_sd without r_fwer
    (fname,) = getattr(m, store)(res, Table, None, out, stepdown=True)
    assert fname == out + "host" + suffix
    lines = open(fname).read().splitlines()
    assert lines[0] == ",".join('"%s"' % c for c in m.ROARY_HEAD + list(getattr(m, columns)) +
                                ["Empirical_p", "Westfall_Young_stepdown_p"])
    assert [l.rsplit(",", 1)[0] for l in lines] == without
    assert [l.rsplit(",", 1)[1] for l in lines[1:]] == ['"0.1"', '"0.5"', '"0.75"']     # rows b, a, c
    # with both: the step-down column is the last
    res["host"]["r_fwer"] = np.array([9, 1, 19, 19])
    (fname,) = getattr(m, store)(res, Table, None, out, stepdown=True)
    both = open(fname).read().splitlines()
    assert both[0] == without[0] + ',"Westfall_Young_p","Westfall_Young_stepdown_p"'
    assert [l.rsplit(",", 2)[0] for l in both] == without
    assert [l.rsplit(",", 2)[1:] for l in both[1:]] == [['"0.1"', '"0.1"'], ['"0.5"', '"0.5"'], ['"1.0"', '"0.75"']]
    # without permutations there is no column, whatever the dict holds
    del res["host"]["r"]
    (fname,) = getattr(m, store)(res, Table, None, out, stepdown=True)
    text = open(fname).read()
    assert "Westfall_Young" not in text and "Empirical_p" not in text


def test_the_entry_points_are_in_the_binding_the_header_and_the_build():
    import __graft_entry__ as ge
    from scoary_amd import _abi, engine
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert _abi.ABI_VERSION == 11 and "spec S23" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\b(?:int|int64_t) %s\(([^;]*)\);" % name, code)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    # the entry points that were there keep their shapes
    assert len(_abi.SIGNATURES["scoary_permute_cat_wy"][1]) == 16
    assert len(_abi.SIGNATURES["scoary_permute_gcmh_wy"][1]) == 14
    assert len(_abi.SIGNATURES["scoary_permute_rank_stepdown"][1]) == 14
    for name in ("cat_stepdown_batch", "cat_stepdown_gather", "gcmh_stepdown_gather", "permute_cat_stepdown",
                 "permute_gcmh_stepdown", "categorical_stepdown", "gcmh_stepdown", "rank_stepdown_order",
                 "rank_stepdown_tail", "r_fwer_max"):
        assert callable(getattr(engine.AssociationEngine, name))
    assert any(s.endswith("scoary_cat_stepdown.hip") for s in ge.HIP_SRCS)
    # the new unit compiles the one text of the planes' walk, of the statistic and of Q
    csrc = os.path.dirname(ge.HIP_SRCS[0])
    with open(os.path.join(csrc, "scoary_cat_stepdown.hip")) as f:
        text = f.read()
    assert '#include "scoary_cat_planes.hpp"' in text and '#include "scoary_gcmh_form.hpp"' in text
    for own in ("void cat_count(", "__int128 cat_mul(", "double gcmh_q(", "double cat_wy_add(", "struct CatStage"):
        assert own not in text, own
    for used in ("cat_wy_add(", "gcmh_q<", "cat_hits(", "count_group(", "cat_launch_plan("):
        assert used in text, used
    if os.path.exists(_abi.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_abi.LIB_PATH)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), name


def test_the_batch_size_keeps_rows_and_gmax_under_the_budget():
    from scoary_amd.engine import AssociationEngine as E
    eng = E.__new__(E)                                   # (the method reads nothing of the engine)
    G, T, N = 2049, 5, 33
    per = 2 * 64 * T * N + 8 * T * 48 * 64               # code rows + gmax (3 supergroups = 48 runs) of 64 permutations
    assert eng.cat_stepdown_batch(G, T, N, 1000, 10 * per) == 640
    assert eng.cat_stepdown_batch(G, T, N, 1000, 10 * per - 1) == 576
    assert eng.cat_stepdown_batch(G, T, N, 1000, 1) == 64
    assert eng.cat_stepdown_batch(G, T, N, 100) == 128 and eng.cat_stepdown_batch(1024, T, N, 64) == 64


def test_resource_rules():
    import __graft_entry__ as ge
    assert [r["name"] for r in ge.CAT_SD_RULES] == ["k_cat_sd_gather", "k_cat_sd_suffix", "k_cat_sd_max",
                                                    "k_cat_sd_count", "k_gcmh_sd_max", "k_gcmh_sd_count"]
    assert all(r["count"] == 1 and r["scratch"] == 0 for r in ge.CAT_SD_RULES)
    assert all(r["cap"] == (("VGPRs",), 128) for r in ge.CAT_SD_RULES[2:])
    assert [r["sgpr_spills"] for r in ge.CAT_SD_RULES] == [0, 0, 18, 18, 44, 44]
    assert ge.CAT_SD_RULES[2]["sgpr_spills"] == ge.CAT_WY_RULES[1]["sgpr_spills"]       # the sibling caps
    assert ge.CAT_SD_RULES[4]["sgpr_spills"] == ge.CAT_WY_RULES[2]["sgpr_spills"]
    ok = {n: {"VGPRs": 92, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0} for n in KERNELS}
    ge.check_kernel_resources(ok, ge.CAT_SD_RULES)
    for n in KERNELS:                                  # scratch or a spill in any of the six fails the build
        for field, what in (("ScratchSize", "scratch 64"), ("SGPRs Spill", "SGPR spills 64"),
                            ("VGPRs Spill", "VGPR spills 64")):
            bad = {k: dict(v, **({field: 64} if k == n else {})) for k, v in ok.items()}
            with pytest.raises(RuntimeError, match=what):
                ge.check_kernel_resources(bad, ge.CAT_SD_RULES)
    for n in HOT:
        with pytest.raises(RuntimeError, match="129 VGPRs > 128"):
            ge.check_kernel_resources({k: dict(v, VGPRs=129 if k == n else 92) for k, v in ok.items()}, ge.CAT_SD_RULES)
    for n, cap in zip(HOT, (18, 18, 44, 44)):          # SGPRs in VGPR lanes: at most the sibling's
        ge.check_kernel_resources({k: dict(v, **({"SGPRs Spill": cap} if k == n else {})) for k, v in ok.items()},
                                  ge.CAT_SD_RULES)
        with pytest.raises(RuntimeError, match="SGPR spills %d" % (cap + 1)):
            ge.check_kernel_resources({k: dict(v, **({"SGPRs Spill": cap + 1} if k == n else {}))
                                       for k, v in ok.items()}, ge.CAT_SD_RULES)
    with pytest.raises(RuntimeError, match="expected 1 k_gcmh_sd_count instance, compiler reported 0"):
        ge.check_kernel_resources({n: ok[n] for n in KERNELS[:5]}, ge.CAT_SD_RULES)
    # the new kernels are in no other family: the kernels of S20 to S22 and of S18 stay one kernel each
    every = (ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES +
             ge.CMH_HOMOG_RULES + ge.FISHER_CHAINS_RULES + ge.RANKSUM_RULES + ge.VANELTEREN_RULES + ge.RANK_WY_RULES +
             ge.RANK_SD_RULES + ge.RANK_SHIFT_RULES + ge.CATEGORICAL_RULES + ge.GCMH_RULES + ge.CAT_WY_RULES)
    for other in every:
        assert not any(other["name"] in n and not (other["exclude"] and other["exclude"] in n) for n in KERNELS), other
    for banned in ("k_cat_permute", "k_cat_maxt", "k_cat_observed", "k_cat_wy_prepare", "k_gcmh_permute",
                   "k_gcmh_maxt", "k_gcmh_observed"):
        assert not any(banned in n for n in KERNELS), banned
    # and each new name falls into exactly its own rule
    for n in KERNELS:
        assert sum(r["name"] in n for r in ge.CAT_SD_RULES) == 1, n
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            res = json.load(f)
        for rules in (ge.CAT_SD_RULES, ge.CAT_WY_RULES, ge.CATEGORICAL_RULES, ge.GCMH_RULES):
            ge.check_kernel_resources(res, rules)
        assert all(n in res for n in KERNELS)
