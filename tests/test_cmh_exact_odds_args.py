"""--cmh-exact-odds / --cmh-exact-level: the argument checks on the command line (they exit before the engine is
touched) and in Setup_results / associate (the same rules as ValueErrors), the place of the three columns and of the
rule row, the binding and the resource rule of the kernel."""
import os

import pytest

from args_cases import COLUMNS, good_strata_file as _strata_file, rule_of, run_refused as _run

FLAG, KW = "--cmh-exact-odds", "cmh_exact_odds"
NO_CMH = "Cannot use --cmh-exact-odds without --cmh FILE. The exact test is taken over the strata of FILE"
NO_PAIRWISE = ("Cannot use --cmh-exact-odds without --no_pairwise. The exact conditional odds ratio is an estimate for "
               "every gene over the strata, beside Fisher's test")
NO_ODDS = ("Cannot use --cmh-exact-level without --cmh-exact-odds. It is the confidence level of the limits of the "
           "exact conditional odds ratio")
BAD_LEVEL = "The confidence level of --cmh-exact-level must be between 0.0 and 1.0 (both excluded)"
NAMES = ["CMH_exact_odds_ratio", "CMH_exact_odds_ratio_lower", "CMH_exact_odds_ratio_upper"]


def test_flag_parsing():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.cmh_exact_odds is False and args.cmh_exact_level is None and m.DEFAULT_EXACT_LEVEL == 0.95
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--cmh", "s.csv", FLAG])
    assert args.cmh_exact_odds is True and args.cmh_exact is False and args.cmh == "s.csv" and args.permute == 0
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--cmh", "s.csv", FLAG, "--cmh-exact",
                                         "--cmh-exact-level", "0.99", "--cmh-fwer", "-e", "100"])
    assert args.cmh_exact_odds and args.cmh_exact and args.cmh_fwer and args.cmh_exact_level == 0.99


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    from scoary_amd import dist, methods as m
    path = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run([FLAG]) == NO_PAIRWISE
    assert run([FLAG, "--cmh", path]).startswith("Cannot use --cmh without --no_pairwise")
    assert run(["--no_pairwise", FLAG]) == NO_CMH
    assert run(["--no_pairwise", FLAG, "--cmh-exact"]) == NO_CMH
    assert run(["--no_pairwise", FLAG, "-e", "100", "--permute-strata", path]) == NO_CMH
    assert run(["--no_pairwise", FLAG, "--cmh", path, "-e", "100", "--permute-early-abort"]) \
        .startswith("Cannot use --cmh together with --permute-early-abort")
    rule = rule_of(FLAG)
    assert list(m._broken_rules(rule, False, 0, False, (), cmh=False)) == [NO_PAIRWISE, NO_CMH]
    assert list(m._broken_rules(rule, True, 0, False, (), cmh=True)) == []         # no permutations needed
    assert list(m._broken_rules(rule, True, 100, True, (), cmh=True)) == []
    monkeypatch.setattr(dist, "world_rank", lambda: (2, 0))
    assert run(["--no_pairwise", FLAG, "--cmh", path]).startswith("Cannot use --cmh under more than one rank")
    assert list(m._broken_rules(rule, True, 0, False, (), cmh=True)) == \
        ["Cannot use --cmh-exact-odds under more than one rank: %s" % rule.one_rank]
    assert list(m._broken_rules(rule, True, 0, False, None, cmh=True)) == \
        ["cmh_exact_odds needs a single process: %s" % rule.one_rank]


def test_the_level_is_refused_outside_its_range_and_without_the_flag(exampledir, tmp_path, monkeypatch):
    path = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    ok = ["--no_pairwise", "--cmh", path]
    assert run(ok + ["--cmh-exact-level", "0.9"]) == NO_ODDS
    assert run(ok + ["--cmh-exact", "--cmh-exact-level", "0.9"]) == NO_ODDS
    for bad in ("0", "1", "0.0", "1.0", "-0.5", "1.5", "95", "nan", "inf"):
        assert run(ok + [FLAG, "--cmh-exact-level", bad]) == BAD_LEVEL, bad
    # the flag's own rules come first
    assert run(["--no_pairwise", FLAG, "--cmh-exact-level", "2"]) == NO_CMH


def test_setup_results_raises_the_same_rules():
    from scoary_amd import methods as m
    for kw in ({}, {"permutations": 100}, {"permutations": 100, "strata": [0, 1]}):
        with pytest.raises(ValueError, match=r"cmh_exact_odds needs cmh \(and its strata\)"):
            m.Setup_results({}, {}, False, cmh_exact_odds=True, **kw)
    with pytest.raises(ValueError, match="cmh needs strata"):
        m.Setup_results({}, {}, False, cmh=True, cmh_exact_odds=True)
    for bad in (0.0, 1.0, -1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match=r"cmh_exact_level must lie inside \(0, 1\)"):
            m.Setup_results({}, {}, False, strata=[0, 1], cmh=True, cmh_exact_odds=True, cmh_exact_level=bad)


def test_the_engine_refuses_the_odds_without_cmh_and_a_level_outside_its_range():
    from scoary_amd.engine import AssociationEngine
    with pytest.raises(ValueError, match=r"cmh_exact_odds=True needs cmh=True"):
        AssociationEngine.associate(None, None, None, None, cmh_exact_odds=True)
    for bad in (0.0, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"cmh_exact_level must lie inside \(0, 1\)"):
            AssociationEngine.associate(None, None, None, None, cmh=True, cmh_exact_odds=True, cmh_exact_level=bad)
        with pytest.raises(ValueError, match=r"the confidence level must lie inside \(0, 1\)"):
            AssociationEngine.cmh_exact_odds(None, None, None, None, {}, level=bad)


def test_columns_come_after_every_other_and_the_existing_pins_hold():
    from scoary_amd import methods as m
    assert m.OPTIONAL_COLUMNS == COLUMNS and [name for name, _key, _count in COLUMNS[len(COLUMNS) - 3:]] == NAMES
    flags = [r.flag for r in m.FLAG_RULES]
    assert flags[len(flags) - 2:] == [FLAG, "--cmh-exact"]                  # checked before --cmh-exact, written after
    assert flags.index("--cmh") < flags.index("--cmh-fwer")
    rule = rule_of(FLAG)
    assert (rule.kw, rule.needs_permutations, rule.no_early_abort, rule.needs_cmh) == (KW, False, False, "cmh_exact")
    assert rule.one_rank == rule_of("--cmh").one_rank
    assert {r.flag: r.needs_cmh for r in m.FLAG_RULES if r.needs_cmh} == {
        "--cmh-fwer": "cmh", "--cmh-fwer-stepdown": "cmh", FLAG: "cmh_exact", "--cmh-exact": "cmh_exact"}
    assert m.RULE_TEXT["cmh_exact"][0] % {"flag": FLAG} == NO_CMH


def test_the_header_of_a_results_file_ends_with_the_three_columns(tmp_path):
    """StoreTraitResult from plain row dicts (no engine): the header, the place of the cells and the spelling of inf
    and nan, which is CMH_odds_ratio's."""
    import csv
    from scoary_amd import methods as m
    rows = {}
    for i, (odds, lo, hi) in enumerate([(2.5, 0.5, 12.0), (float("inf"), 1.5, float("inf")),
                                        (float("nan"), 0.0, float("inf")), (0.0, 0.0, 0.75)]):
        rows["gene%d" % i] = {"NUGN": "", "Annotation": "x", "tpgp": 1, "tngp": 2, "tpgn": 3, "tngn": 4, "sens": 25.0,
                              "spes": 66.0, "OR": 0.66, "p_v": 0.1 * (i + 1), "B_p": 0.4, "BH_p": 0.4,
                              "CMH_p": 0.3, "CMH_odds_ratio": odds, "CMH_exact_p": 0.31, "CMH_exact_odds_ratio": odds,
                              "CMH_exact_odds_ratio_lower": lo, "CMH_exact_odds_ratio_upper": hi}
    name = m.StoreTraitResult(rows, "trait", None, {"I": 1.0}, None, None, None, str(tmp_path) + "/", 0, 1, True, None,
                              [], ["Gene", "Non-unique Gene name", "Annotation"])
    with open(name, newline="") as f:
        table = list(csv.reader(f))
    assert table[0][-6:] == ["CMH_p", "CMH_odds_ratio", "CMH_exact_p"] + NAMES
    assert [r[-3:] for r in table[1:]] == [["2.5", "0.5", "12.0"], ["inf", "1.5", "inf"], ["nan", "0.0", "inf"],
                                           ["0.0", "0.0", "0.75"]]
    assert [r[-5] for r in table[1:]] == [r[-3] for r in table[1:]]            # CMH_odds_ratio's spelling
    for gene in rows.values():                                                  # without the keys: today's header
        for k in NAMES:
            del gene[k]
    name = m.StoreTraitResult(rows, "plain", None, {"I": 1.0}, None, None, None, str(tmp_path) + "/", 0, 1, True, None,
                              [], ["Gene", "Non-unique Gene name", "Annotation"])
    with open(name, newline="") as f:
        assert next(csv.reader(f))[-3:] == ["CMH_p", "CMH_odds_ratio", "CMH_exact_p"]


def test_binding_declares_the_entry_point():
    from scoary_amd import _abi
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert "scoary_cmh_exact_odds(" in header and "spec S13" in header and _abi.ABI_VERSION == 11
    restype, args = _abi.SIGNATURES["scoary_cmh_exact_odds"]
    exact = _abi.SIGNATURES["scoary_cmh_exact"][1]
    assert len(args) == len(exact) and sum(a is __import__("ctypes").c_double for a in args) == 1


def test_kernels_compiled_to_their_resource_rules():
    import json
    import __graft_entry__ as ge
    if not os.path.exists(ge.HIP_RESOURCES):
        ge.build()
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    hit = [v for k, v in res.items() if "k_cmh_odds_exact" in k]
    assert len(hit) == 1
    assert hit[0]["ScratchSize"] == 0 and hit[0]["VGPRs Spill"] == 0 and hit[0]["SGPRs Spill"] == 0
    (rule,) = ge.CMH_EXACT_ODDS_RULES
    assert rule["name"] == "k_cmh_odds_exact" and hit[0]["VGPRs"] <= rule["cap"][1] <= 168     # three waves per SIMD
    # k_cmh_exact is still one kernel, under its own rule, and no rule's name catches the other kernel
    assert len([k for k in res if "k_cmh_exact" in k]) == 1
    assert ge.CMH_EXACT_RULES[0]["name"] not in "k_cmh_odds_exactE" and rule["name"] not in "k_cmh_exactE"
    for other in ge.CMH_RULES:
        assert other["name"] not in "k_cmh_odds_exactE"
    ge.check_kernel_resources(res, ge.RESOURCE_RULES + ge.CMH_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES)
