"""--quantitative-shift and --quantitative-shift-level: their refusals on the command line (they exit before the
engine is touched) and in Ranksum_results, the 1e150 rule, the level's default, the three columns and where they
stand with and without the permutation columns, and what the feature adds to the binding, the header and the build
(spec S19)."""
import os
import re

import numpy as np
import pytest

from args_cases import run_refused as _run

FLAG, LEVEL = "--quantitative-shift", "--quantitative-shift-level"
NEEDS_QUANTITATIVE = ("Cannot use --quantitative-shift without --quantitative. It is the shift of the measured traits "
                      "with a gene, next to the rank-sum test")
NEEDS_FLAG = ("Cannot use --quantitative-shift-level without --quantitative-shift. It is the confidence level of "
              "the limits of the Hodges-Lehmann shift")
BAD_LEVEL = "The confidence level of --quantitative-shift-level must be between 0.0 and 1.0 (both excluded)"
TOO_LARGE = ("Cannot use --quantitative-shift with a value above 1e150 in magnitude: the difference of two such "
             "values could overflow")
COLUMNS = ["Rank_sum_shift", "Rank_sum_shift_lower", "Rank_sum_shift_upper"]
ENTRY_POINTS = {"scoary_ranksum_shift": 16, "scoary_rank_shift_waves": 1}
KERNEL = "_ZN12_GLOBAL__N_112k_rank_shiftEPKjliiiiPKdPKiS1_S5_S3_dPdS6_S6_Pl"


def _qfile(tmp_path, text="Name,mic\nA,1.5\n", name="q.csv"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def test_flag_is_off_by_default_and_the_level_is_95_percent():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.quantitative_shift is False and args.quantitative_shift_level is None
    assert m._shift_level(args) == 0.95 == m.RANK_SHIFT_LEVEL
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", "--quantitative", "q.csv", FLAG])
    assert (args.quantitative, args.quantitative_shift, args.permute) == ("q.csv", True, 0)     # no permutations
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", "--quantitative", "q.csv", FLAG,
                                         LEVEL, "0.9"])
    assert m._shift_level(args) == 0.9
    import inspect
    sig = inspect.signature(m.Ranksum_results).parameters
    assert sig["shift"].default is False and sig["shift_level"].default == 0.95


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    q = _qfile(tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run(["--no_pairwise", FLAG]) == NEEDS_QUANTITATIVE
    assert run(["--no_pairwise", FLAG, LEVEL, "0.9"]) == NEEDS_QUANTITATIVE
    assert run(["--no_pairwise", "--quantitative", q, LEVEL, "0.9"]) == NEEDS_FLAG
    assert run(["--no_pairwise", LEVEL, "0.9"]) == NEEDS_FLAG
    for bad in ("0", "1", "1.5", "-0.2", "nan"):
        assert run(["--no_pairwise", "--quantitative", q, FLAG, LEVEL, bad]) == BAD_LEVEL, bad
    # the rules of --quantitative and of the Westfall-Young flags come first
    assert run(["--quantitative", q, FLAG]).startswith("Cannot use --quantitative without --no_pairwise")
    assert run(["--no_pairwise", "--quantitative", q, "--quantitative-fwer", FLAG]).startswith(
        "Cannot use --quantitative-fwer without --permute")


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    vals = np.array([[1.0, 2.0, np.nan]])
    for bad in (0.0, 1.0, -0.5, 2.0, float("nan")):
        with pytest.raises(ValueError) as e:
            m.Ranksum_results(None, ["x"], vals, shift=True, shift_level=bad)
        assert str(e.value) == BAD_LEVEL
    for big in (1.0000001e150, -2e150, 1e300):
        with pytest.raises(ValueError) as e:
            m.Ranksum_results(None, ["x"], np.array([[1.0, big, np.nan]]), shift=True)
        assert str(e.value) == TOO_LARGE
    with pytest.raises(ValueError, match="quantitative traits need no_pairwise"):
        m.Ranksum_results(None, ["x"], vals, shift=True, no_pairwise=False)
    with pytest.raises(ValueError) as e:                                     # the Westfall-Young rules are first
        m.Ranksum_results(None, ["x"], vals, shift=True, shift_level=7.0, fwer=True)
    assert str(e.value) == m.RANK_WY_TEXT["permute"]
    assert m.RANK_SHIFT_TEXT == {"quantitative": NEEDS_QUANTITATIVE, "level_flag": NEEDS_FLAG, "level": BAD_LEVEL,
                                 "magnitude": TOO_LARGE}
    assert [key for key, _broken in m.RANK_SHIFT_FLAG_RULES] == ["quantitative", "level_flag", "level", "magnitude"]
    assert list(m._rank_shift_refusals(False, False, None)) == []
    assert list(m._rank_shift_refusals(True, True, None, vals)) == []
    assert list(m._rank_shift_refusals(True, True, 0.5, np.array([[1e150, -1e150]]))) == []      # at the bound: taken
    assert list(m._rank_shift_refusals(True, False, 3.0, np.array([[2e150]]))) == [NEEDS_QUANTITATIVE, BAD_LEVEL,
                                                                                   TOO_LARGE]
    assert list(m._rank_shift_refusals(False, True, 0.9)) == [NEEDS_FLAG]
    # without the flag a large value is no reason to refuse: the rank-sum test ranks it
    assert list(m._rank_shift_refusals(False, True, None, np.array([[2e150]]))) == []


def test_the_plan_refuses_what_could_overflow():
    from scoary_amd import engine as e
    assert e.SHIFT_MAX_ABS == 1e150
    with pytest.raises(ValueError, match="1e150"):
        e.shift_rows(np.array([[0.0, -1.1e150]]))
    xs, pos = e.shift_rows(np.array([[3.0, np.nan, -0.0, 1e150, -2.0, 3.0]]))
    assert xs.tolist() == [[-2.0, 0.0, 3.0, 3.0, 1e150, 0.0]] and pos.tolist() == [[4, 2, 0, 5, 3, 0]]
    assert not np.signbit(xs).any() or xs[0, 0] == -2.0
    assert np.signbit(xs[0, 1]) == False                                     # noqa: E712  (-0.0 is stored as +0.0)
    assert xs.dtype == np.float64 and pos.dtype == np.int32


def test_the_binary_steps_tables_do_not_know_the_flag():
    from scoary_amd import methods as m
    assert not any(rule.flag in (FLAG, LEVEL) for rule in m.ALL_RULES)
    assert [c for c, _key in m.RANK_SHIFT_COLUMNS] == COLUMNS
    assert not set(COLUMNS) & set(m.RANKSUM_COLUMNS + m.VANELTEREN_COLUMNS)


def test_the_columns_stand_behind_benjamini_h_p_and_the_permutation_columns_stay_last(tmp_path, monkeypatch):
    from scoary_amd import methods as m

    class Table:
        ids, nugn, annotation, strains = ["a", "b_|_nb_|_ab", "c", "d"], ["na", "", "nc", "nd"], ["x", "", "y", "z"], []
    monkeypatch.setattr(m, "_as_table", lambda g: g)
    base = dict(n=10, m=np.array([3, 4, 5, 0]), auc=np.array([0.75, 0.25, 0.5, 0.5]),
                p=np.array([0.04, 0.01, 0.04, 1.0]), testable=np.array([True, True, True, False]))
    hl = dict(shift=np.array([1.5, -0.25, 0.0, 0.0]), shift_lower=np.array([-np.inf, -1.0, -2.0, -np.inf]),
              shift_upper=np.array([np.inf, 0.5, 1e-300, np.inf]))
    out = str(tmp_path) + os.sep
    head = m.ROARY_HEAD + list(m.RANKSUM_COLUMNS)
    assert head[-1] == "Benjamini_H_p"
    nh = len(head)
    for perm in ({}, dict(r=np.array([4, 0, 9, 20]), permutations=19),
                 dict(r=np.array([4, 0, 9, 20]), permutations=19, r_fwer=np.array([9, 1, 19, 19])),
                 dict(r=np.array([4, 0, 9, 20]), permutations=19, r_sd=np.array([7, 1, 19, 19])),
                 dict(r=np.array([4, 0, 9, 20]), permutations=19, r_fwer=np.array([9, 1, 19, 19]),
                      r_sd=np.array([7, 1, 19, 19]))):
        tail = (["Empirical_p"] if "r" in perm else []) + (["Westfall_Young_p"] if "r_fwer" in perm else []) + \
            (["Westfall_Young_stepdown_p"] if "r_sd" in perm else [])
        (fname,) = m.StoreRanksumResults({"mic": dict(base, **perm)}, Table, None, out)
        plain = [line.split(",") for line in open(fname).read().splitlines()]
        (fname,) = m.StoreRanksumResults({"mic": dict(base, **perm, **hl)}, Table, None, out)
        got = [line.split(",") for line in open(fname).read().splitlines()]
        assert got[0] == ['"%s"' % c for c in head + COLUMNS + tail]
        assert [row[:nh] + row[nh + 3:] for row in got] == plain             # every other cell: the file without
        assert [row[nh:nh + 3] for row in got[1:]] == [['"-0.25"', '"-1.0"', '"0.5"'],           # rows b, a, c
                                                       ['"1.5"', '"-inf"', '"inf"'], ['"0.0"', '"-2.0"', '"1e-300"']]
    # the van Elteren file takes no such columns: its results never hold the keys
    (fname,) = m.StoreVanElterenResults({"mic": dict(base)}, Table, None, out)
    assert "shift" not in open(fname).read()
    # two of the three keys are no column
    (fname,) = m.StoreRanksumResults({"mic": dict(base, shift=hl["shift"], shift_lower=hl["shift_lower"])}, Table, None, out)
    assert "shift" not in open(fname).read()


def test_the_entry_points_are_in_the_binding_the_header_and_the_build():
    import __graft_entry__ as ge
    from scoary_amd import _abi
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert _abi.ABI_VERSION == 11 and re.search(r"#define SCOARY_ABI_VERSION 11\b", header) and "spec S19" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint(?:64_t)? %s\(([^;]*)\);" % name, code)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    import ctypes
    assert _abi.SIGNATURES["scoary_ranksum_shift"][1][7] is ctypes.c_double               # zq
    assert len(_abi.SIGNATURES["scoary_ranksum_var"][1]) == 9 and len(_abi.SIGNATURES["scoary_ranksum"][1]) == 13
    assert any(s.endswith("scoary_rank_shift.hip") for s in ge.HIP_SRCS)
    if os.path.exists(_abi.LIB_PATH):
        lib = ctypes.CDLL(_abi.LIB_PATH)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), name
        lib.scoary_rank_shift_waves.restype, lib.scoary_rank_shift_waves.argtypes = ctypes.c_int64, [ctypes.c_int64]
        assert [lib.scoary_rank_shift_waves(n) for n in (0, 1, 2000, 16320, 16321)] == [0, 16, 16, 1, 0]


def test_resource_rules():
    import __graft_entry__ as ge
    (rule,) = ge.RANK_SHIFT_RULES
    assert rule["name"] == "k_rank_shift" and rule["scratch"] == 0 and rule["cap"] == (("VGPRs",), 64)
    ok = {KERNEL: {"VGPRs": 39, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": rule["sgpr_spills"]}}
    ge.check_kernel_resources(ok, ge.RANK_SHIFT_RULES)
    for field, text in (("ScratchSize", "scratch 8"), ("VGPRs Spill", "VGPR spills 8"), ("VGPRs", "65 VGPRs > 64"),
                        ("SGPRs Spill", "SGPR spills %d" % (rule["sgpr_spills"] + 1))):
        bad = {KERNEL: dict(ok[KERNEL], **{field: int(re.search(r"\d+", text).group())})}
        with pytest.raises(RuntimeError, match=text):
            ge.check_kernel_resources(bad, ge.RANK_SHIFT_RULES)
    with pytest.raises(RuntimeError, match="expected 1 k_rank_shift instance, compiler reported 0"):
        ge.check_kernel_resources({}, ge.RANK_SHIFT_RULES)
    every = (ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES + ge.RANKSUM_RULES + ge.VANELTEREN_RULES +
             ge.RANK_WY_RULES + ge.RANK_SD_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES + ge.CMH_HOMOG_RULES +
             ge.FISHER_CHAINS_RULES)
    for other in every:                                  # the new kernel is in no other family
        assert not (other["name"] in KERNEL and not (other["exclude"] and other["exclude"] in KERNEL)), other
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            res = json.load(f)
        ge.check_kernel_resources(res, every + ge.RANK_SHIFT_RULES)
