"""--quantitative-fwer-stepdown: its refusals on the command line (they exit before the engine is touched) and in
Ranksum_results / VanElteren_results, and their order; its column, the last one with and without --quantitative-fwer;
and what the feature adds to the binding, the header and the build (spec S18)."""
import os
import re

import numpy as np
import pytest

from args_cases import good_strata_file as _strata_file, run_refused as _run

FLAG = "--quantitative-fwer-stepdown"
NEEDS_QUANTITATIVE = ("Cannot use --quantitative-fwer-stepdown without --quantitative. It is the step-down family-wise "
                      "p of the rank tests of the measured traits")
NEEDS_PERMUTE = ("Cannot use --quantitative-fwer-stepdown without --permute X, X >= 10. The family-wise p is counted "
                 "over the permutations of the values")
ENTRY_POINTS = {"scoary_rank_stepdown_scratch_bytes": 5, "scoary_rank_stepdown_gather": 11,
                "scoary_permute_rank_stepdown": 14}
KERNELS = ["_ZN12_GLOBAL__N_116k_rank_sd_gatherEPK15HIP_vector_typeIjLj4EEPKiPKdS7_S5_iliPS1_PdS9_Pi",
           "_ZN12_GLOBAL__N_116k_rank_sd_suffixEPdilllS0_l",
           "_ZN12_GLOBAL__N_113k_rank_sd_maxEPKhliiiS1_PKiPKdiliiiPiPd",
           "_ZN12_GLOBAL__N_115k_rank_sd_countEPKhliiiS1_PKdS3_iliiiPiPd"]


def _qfile(tmp_path, text="Name,mic\nA,1.5\n", name="q.csv"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.quantitative_fwer_stepdown is False and args.quantitative_fwer is False
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", "--quantitative", "q.csv",
                                         "-e", "100", FLAG])
    assert (args.quantitative, args.quantitative_fwer_stepdown, args.quantitative_fwer, args.permute) == \
        ("q.csv", True, False, 100)                                          # either flag works without the other


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    q = _qfile(tmp_path)
    strata = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run(["--no_pairwise", FLAG]) == NEEDS_QUANTITATIVE
    assert run(["--no_pairwise", "-e", "100", FLAG]) == NEEDS_QUANTITATIVE
    assert run(["--no_pairwise", "--quantitative", q, FLAG]) == NEEDS_PERMUTE
    assert run(["--no_pairwise", "--quantitative", q, "--quantitative-strata", strata, FLAG]) == NEEDS_PERMUTE
    # the rules of --quantitative come first, then those of --quantitative-fwer, then these
    assert run(["--quantitative", q, "-e", "100", FLAG]).startswith("Cannot use --quantitative without --no_pairwise")
    assert run(["--no_pairwise", "--quantitative-fwer", FLAG]).startswith("Cannot use --quantitative-fwer without "
                                                                          "--quantitative.")
    assert run(["--no_pairwise", "--quantitative", q, "--quantitative-fwer", FLAG]).startswith(
        "Cannot use --quantitative-fwer without --permute")
    # --permute 1 .. 9 is refused by --permute's own rule or by this one, never run
    assert isinstance(run(["--no_pairwise", "--quantitative", q, "-e", "9", FLAG]), str)


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    vals, st = np.zeros((1, 3)), np.zeros(3, dtype=np.int64)
    for perms in (0, 9):
        with pytest.raises(ValueError) as e:
            m.Ranksum_results(None, ["x"], vals, permutations=perms, stepdown=True)
        assert str(e.value) == NEEDS_PERMUTE
        with pytest.raises(ValueError) as e:
            m.VanElteren_results(None, ["x"], vals, st, permutations=perms, stepdown=True)
        assert str(e.value) == NEEDS_PERMUTE
        with pytest.raises(ValueError) as e:                                 # --quantitative-fwer's rule is first
            m.Ranksum_results(None, ["x"], vals, permutations=perms, fwer=True, stepdown=True)
        assert str(e.value) == m.RANK_WY_TEXT["permute"]
    with pytest.raises(ValueError, match="quantitative traits need no_pairwise"):
        m.Ranksum_results(None, ["x"], vals, stepdown=True, no_pairwise=False)
    assert m.RANK_SD_TEXT == {"quantitative": NEEDS_QUANTITATIVE, "permute": NEEDS_PERMUTE}
    assert [key for key, _broken in m.RANK_SD_FLAG_RULES] == ["quantitative", "permute"]
    assert list(m._rank_sd_refusals(False, False, 0)) == []
    assert list(m._rank_sd_refusals(True, False, 0)) == [NEEDS_QUANTITATIVE, NEEDS_PERMUTE]
    assert list(m._rank_sd_refusals(True, True, 9)) == [NEEDS_PERMUTE]
    assert list(m._rank_sd_refusals(True, True, 10)) == []


def test_the_binary_steps_tables_do_not_know_the_flag():
    from scoary_amd import methods as m
    assert not any(rule.flag == FLAG for rule in m.ALL_RULES) and not any(rule.flag == FLAG for rule in m.FLAG_RULES)
    assert "Westfall_Young_stepdown_p" not in m.RANKSUM_COLUMNS + m.VANELTEREN_COLUMNS


@pytest.mark.parametrize("store, columns, suffix", (("StoreRanksumResults", "RANKSUM_COLUMNS", ".ranksum.results.csv"),
                                                    ("StoreVanElterenResults", "VANELTEREN_COLUMNS",
                                                     ".vanelteren.results.csv")))
def test_the_column_is_the_last_with_and_without_the_single_step_one(tmp_path, monkeypatch, store, columns, suffix):
    from scoary_amd import methods as m

    class Table:
        ids, nugn, annotation, strains = ["a", "b_|_nb_|_ab", "c", "d"], ["na", "", "nc", "nd"], ["x", "", "y", "z"], []
    monkeypatch.setattr(m, "_as_table", lambda g: g)
    res = {"mic": dict(n=10, m=np.array([3, 4, 5, 0]), auc=np.array([0.75, 0.25, 0.5, 0.5]),
                       p=np.array([0.04, 0.01, 0.04, 1.0]), testable=np.array([True, True, True, False]),
                       r=np.array([4, 0, 9, 20]), permutations=19)}
    out = str(tmp_path) + os.sep
    head = m.ROARY_HEAD + list(getattr(m, columns)) + ["Empirical_p"]
    (fname,) = getattr(m, store)(res, Table, None, out)
    plain = open(fname).read().splitlines()
    # without --quantitative-fwer: the new column follows Empirical_p
    res["mic"]["r_sd"] = np.array([7, 1, 19, 19])
    (fname,) = getattr(m, store)(res, Table, None, out)
    assert fname == out + "mic" + suffix
    lines = open(fname).read().splitlines()
    assert lines[0] == ",".join('"%s"' % c for c in head + ["Westfall_Young_stepdown_p"])
    assert [l.rsplit(",", 1)[0] for l in lines] == plain
    assert [l.rsplit(",", 1)[1] for l in lines[1:]] == ['"0.1"', '"0.4"', '"1.0"']     # rows b, a, c
    # with it: behind Westfall_Young_p, and that file is the single-step file plus one cell per row
    res["mic"]["r_fwer"] = np.array([9, 1, 19, 19])
    (fname,) = getattr(m, store)(res, Table, None, out)
    both = open(fname).read().splitlines()
    del res["mic"]["r_sd"]
    (fname,) = getattr(m, store)(res, Table, None, out)
    single = open(fname).read().splitlines()
    assert both[0] == ",".join('"%s"' % c for c in head + ["Westfall_Young_p", "Westfall_Young_stepdown_p"])
    assert [l.rsplit(",", 1)[0] for l in both] == single
    assert [l.rsplit(",", 1)[1] for l in both[1:]] == ['"0.1"', '"0.4"', '"1.0"']
    assert [l.rsplit(",", 1)[1] for l in single[1:]] == ['"0.1"', '"0.5"', '"1.0"']
    # without permutations there is no column, whatever the dict holds
    res["mic"]["r_sd"] = np.array([7, 1, 19, 19])
    del res["mic"]["r"]
    (fname,) = getattr(m, store)(res, Table, None, out)
    assert "Westfall_Young" not in open(fname).read() and "Empirical_p" not in open(fname).read()


def test_the_entry_points_are_in_the_binding_the_header_and_the_build():
    import __graft_entry__ as ge
    from scoary_amd import _abi
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert _abi.ABI_VERSION == 11 and "spec S18" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint(?:64_t)? %s\(([^;]*)\);" % name, code)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    # the entry points that were there keep their shapes
    assert len(_abi.SIGNATURES["scoary_permute_rank_wy"][1]) == 14
    assert len(_abi.SIGNATURES["scoary_permute_ranksum"][1]) == 10
    assert any(s.endswith("scoary_rank_stepdown.hip") for s in ge.HIP_SRCS)
    assert any(s.endswith("scoary_rank_wy.hip") for s in ge.HIP_SRCS)
    if os.path.exists(_abi.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_abi.LIB_PATH)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), name


def test_resource_rules():
    import __graft_entry__ as ge
    assert [r["name"] for r in ge.RANK_SD_RULES] == ["k_rank_sd_gather", "k_rank_sd_suffix", "k_rank_sd_max",
                                                     "k_rank_sd_count"]
    for rule in ge.RANK_SD_RULES[2:]:
        assert rule["cap"] == (("VGPRs", "AGPRs"), 256) == ge.RANKSUM_RULES[2]["cap"]
        assert rule["sgpr_spills"] == 2 == ge.RANKSUM_RULES[2]["sgpr_spills"] and rule["scratch"] == 0
    for rule in ge.RANK_SD_RULES[:2]:
        assert rule["scratch"] == 0 and rule["sgpr_spills"] == 0
    ok = {n: {"VGPRs": 200, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 2 * ("_max" in n or "_count" in n)}
          for n in KERNELS}
    ge.check_kernel_resources(ok, ge.RANK_SD_RULES)
    for gemm in KERNELS[2:]:
        for field, text in (("ScratchSize", "scratch 8"), ("VGPRs Spill", "VGPR spills 8"),
                            ("SGPRs Spill", "SGPR spills 3")):
            bad = {k: dict(v, **({field: int(text.split()[-1])} if k == gemm else {})) for k, v in ok.items()}
            with pytest.raises(RuntimeError, match=text):
                ge.check_kernel_resources(bad, ge.RANK_SD_RULES)
        with pytest.raises(RuntimeError, match="200 VGPRs \\+ 57 AGPRs > 256"):
            ge.check_kernel_resources({k: dict(v, AGPRs=57 if k == gemm else 0) for k, v in ok.items()},
                                      ge.RANK_SD_RULES)
    for small in KERNELS[:2]:
        with pytest.raises(RuntimeError, match="scratch 8"):
            ge.check_kernel_resources({k: dict(v, ScratchSize=8 if k == small else 0) for k, v in ok.items()},
                                      ge.RANK_SD_RULES)
    with pytest.raises(RuntimeError, match="expected 1 k_rank_sd_count instance, compiler reported 0"):
        ge.check_kernel_resources({n: ok[n] for n in KERNELS[:3]}, ge.RANK_SD_RULES)
    # the new kernels are in no other family: the existing rules match by substring and count instances
    every = (ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES + ge.RANKSUM_RULES + ge.VANELTEREN_RULES +
             ge.RANK_WY_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES + ge.CMH_HOMOG_RULES +
             ge.FISHER_CHAINS_RULES)
    for other in every:
        assert not any(other["name"] in n and not (other["exclude"] and other["exclude"] in n) for n in KERNELS), other
    for word in ("k_rank_maxt", "k_permute_ranksum", "k_ranksum", "k_stepdown_minp"):
        assert not any(word in n for n in KERNELS)
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            res = json.load(f)
        ge.check_kernel_resources(res, ge.RANK_SD_RULES)
        ge.check_kernel_resources(res, ge.RANK_WY_RULES)
        ge.check_kernel_resources(res, ge.RANKSUM_RULES)
