"""--cmh-homogeneity: the argument checks on the command line (they exit before the engine is touched) and in
Setup_results / associate (the same rules as ValueErrors), the place of the column and of the rule row beside the
pinned tables, the binding and the resource rule of the kernel."""
import os

import pytest

from args_cases import COLUMNS, good_strata_file as _strata_file, run_refused as _run

FLAG, KW, NAME = "--cmh-homogeneity", "cmh_homogeneity", "CMH_homogeneity_p"
NO_CMH = ("Cannot use --cmh-homogeneity without --cmh FILE. The odds ratios are compared across the strata of FILE")
NO_PAIRWISE = ("Cannot use --cmh-homogeneity without --no_pairwise. The Breslow-Day test of homogeneity is a test of "
               "every gene over the strata, beside Fisher's")
OTHER_FLAGS = ["--permute-fwer", "--permute-fwer-stepdown", "--cmh-fwer", "--cmh-fwer-stepdown", "--cmh-exact",
               "--cmh-exact-odds", "--permute-early-abort"]


def test_flag_is_off_by_default_and_combines_with_every_other_flag():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.cmh_homogeneity is False
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--cmh", "s.csv", FLAG])
    assert args.cmh_homogeneity is True and args.cmh == "s.csv" and args.permute == 0 and args.cmh_exact is False
    for other in OTHER_FLAGS:
        args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--cmh", "s.csv", FLAG, other, "-e", "100"])
        assert args.cmh_homogeneity is True and getattr(args, other[2:].replace("-", "_")) is True
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--cmh", "s.csv", FLAG, "-e", "100",
                                         "--cmh-exact-level", "0.9"] + OTHER_FLAGS[:-1])
    assert args.cmh_homogeneity and args.cmh_exact_odds and args.cmh_fwer_stepdown and args.cmh_exact_level == 0.9
    # every combination passes the rules of the flag itself (no permutations needed, indifferent to early abort)
    (rule,) = m.HOMOGENEITY_RULES
    for permutations in (0, 100):
        for early_abort in (False, True):
            assert list(m._broken_rules(rule, True, permutations, early_abort, (), cmh=True)) == []


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    from scoary_amd import dist, methods as m
    path = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run([FLAG]) == NO_PAIRWISE
    assert run(["--no_pairwise", FLAG]) == NO_CMH
    assert run(["--no_pairwise", FLAG, "-e", "100", "--permute-strata", path]) == NO_CMH
    # the rules of the other flags come first
    assert run([FLAG, "--cmh", path]).startswith("Cannot use --cmh without --no_pairwise")
    assert run(["--no_pairwise", FLAG, "--cmh-exact"]).startswith("Cannot use --cmh-exact without --cmh FILE")
    assert run(["--no_pairwise", FLAG, "--cmh", path, "-e", "100", "--permute-early-abort"]) \
        .startswith("Cannot use --cmh together with --permute-early-abort")
    (rule,) = m.HOMOGENEITY_RULES
    assert list(m._broken_rules(rule, False, 0, False, (), cmh=False)) == [NO_PAIRWISE, NO_CMH]
    monkeypatch.setattr(dist, "world_rank", lambda: (2, 0))
    assert run(["--no_pairwise", FLAG, "--cmh", path]).startswith("Cannot use --cmh under more than one rank")
    assert list(m._broken_rules(rule, True, 0, False, (), cmh=True)) == \
        ["Cannot use --cmh-homogeneity under more than one rank: %s" % rule.one_rank]
    assert list(m._broken_rules(rule, True, 0, False, None, cmh=True)) == \
        ["cmh_homogeneity needs a single process: %s" % rule.one_rank]


def test_setup_results_raises_the_same_rules():
    from scoary_amd import methods as m
    for kw in ({}, {"permutations": 100}, {"permutations": 100, "strata": [0, 1]}, {"early_abort": True}):
        with pytest.raises(ValueError, match=r"cmh_homogeneity needs cmh \(and its strata\)"):
            m.Setup_results({}, {}, False, cmh_homogeneity=True, **kw)
    with pytest.raises(ValueError, match="cmh needs strata"):
        m.Setup_results({}, {}, False, cmh=True, cmh_homogeneity=True)
    # the other flags' rules are raised before this one's
    with pytest.raises(ValueError, match=r"cmh_exact needs cmh \(and its strata\)"):
        m.Setup_results({}, {}, False, cmh_homogeneity=True, cmh_exact=True)


def test_the_engine_refuses_the_test_without_cmh():
    from scoary_amd.engine import AssociationEngine
    with pytest.raises(ValueError, match=r"cmh_homogeneity=True needs cmh=True \(and its strata\)"):
        AssociationEngine.associate(None, None, None, None, cmh_homogeneity=True)
    with pytest.raises(ValueError, match=r"cmh_homogeneity=True needs cmh=True"):
        AssociationEngine.associate(None, None, None, None, permutations=100, cmh_homogeneity=True)


def test_the_pinned_tables_hold_and_the_new_rows_stand_beside_them():
    from scoary_amd import methods as m
    assert m.OPTIONAL_COLUMNS == COLUMNS
    assert m.HOMOGENEITY_COLUMNS == ((NAME, "cmh_homog_p", False),)
    assert m.ALL_COLUMNS == COLUMNS + m.HOMOGENEITY_COLUMNS
    flags = [r.flag for r in m.FLAG_RULES]
    assert flags == ["--permute-fwer", "--permute-fwer-stepdown", "--cmh", "--permute-strata", "--cmh-fwer",
                     "--cmh-fwer-stepdown", "--cmh-exact-odds", "--cmh-exact"]
    assert {r.flag: r.needs_cmh for r in m.FLAG_RULES if r.needs_cmh} == {
        "--cmh-fwer": "cmh", "--cmh-fwer-stepdown": "cmh", "--cmh-exact-odds": "cmh_exact", "--cmh-exact": "cmh_exact"}
    (rule,) = m.HOMOGENEITY_RULES
    assert m.ALL_RULES == m.FLAG_RULES + (rule,)                              # checked after the others
    assert (rule.flag, rule.kw, rule.needs_permutations, rule.no_early_abort, rule.needs_cmh) == \
        (FLAG, KW, False, False, "cmh_homogeneity")
    (cmh_rule,) = [r for r in m.FLAG_RULES if r.flag == "--cmh"]
    assert rule.one_rank == cmh_rule.one_rank
    assert m.RULE_TEXT["cmh_homogeneity"][0] % {"flag": FLAG} == NO_CMH
    assert m.RULE_TEXT["cmh_homogeneity"][1] % {"kw": KW} == "cmh_homogeneity needs cmh (and its strata)"


def test_the_header_of_a_results_file_ends_with_the_column(tmp_path):
    """StoreTraitResult from plain row dicts (no engine): the header, the place of the cells and the spelling of nan,
    which is CMH_odds_ratio's."""
    import csv
    from scoary_amd import methods as m
    rows = {}
    for i, (odds, hp) in enumerate([(2.5, 0.25), (float("inf"), 1.0), (float("nan"), float("nan")), (0.5, 1.5e-300)]):
        rows["gene%d" % i] = {"NUGN": "", "Annotation": "x", "tpgp": 1, "tngp": 2, "tpgn": 3, "tngn": 4, "sens": 25.0,
                              "spes": 66.0, "OR": 0.66, "p_v": 0.1 * (i + 1), "B_p": 0.4, "BH_p": 0.4,
                              "CMH_p": 0.3, "CMH_odds_ratio": odds, "CMH_exact_p": 0.31, "CMH_exact_odds_ratio": odds,
                              "CMH_exact_odds_ratio_lower": 0.0, "CMH_exact_odds_ratio_upper": float("inf"), NAME: hp}
    args = (None, {"I": 1.0}, None, None, None, str(tmp_path) + "/", 0, 1, True, None, [],
            ["Gene", "Non-unique Gene name", "Annotation"])
    with open(m.StoreTraitResult(rows, "trait", *args), newline="") as f:
        table = list(csv.reader(f))
    assert table[0][-7:] == ["CMH_p", "CMH_odds_ratio", "CMH_exact_p", "CMH_exact_odds_ratio",
                             "CMH_exact_odds_ratio_lower", "CMH_exact_odds_ratio_upper", NAME]
    assert [r[-1] for r in table[1:]] == ["0.25", "1.0", "nan", "1.5e-300"]
    assert table[3][-1] == table[3][-6] == "nan"                                # CMH_odds_ratio's spelling
    for gene in rows.values():                                                  # without the key: today's header
        del gene[NAME]
    with open(m.StoreTraitResult(rows, "plain", *args), newline="") as f:
        assert next(csv.reader(f)) == table[0][:-1]


def test_binding_declares_the_entry_point():
    from scoary_amd import _abi
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert "scoary_cmh_homogeneity(" in header and "spec S14" in header and _abi.ABI_VERSION == 11
    assert "#define SCOARY_ABI_VERSION 11" in header
    _restype, args = _abi.SIGNATURES["scoary_cmh_homogeneity"]
    assert len(args) == 19 and args[8:12] == _abi.SIGNATURES["scoary_cmh"][1][8:12]        # G, T, N, S


def test_kernels_compiled_to_their_resource_rules():
    import json
    import __graft_entry__ as ge
    if not os.path.exists(ge.HIP_RESOURCES):
        ge.build()
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    hit = [v for k, v in res.items() if "k_cmh_homog" in k]
    assert len(hit) == 1
    assert hit[0]["ScratchSize"] == 0 and hit[0]["VGPRs Spill"] == 0 and hit[0]["SGPRs Spill"] == 0
    (rule,) = ge.CMH_HOMOG_RULES
    assert rule["name"] == "k_cmh_homog" and hit[0]["VGPRs"] <= rule["cap"][1] <= 128
    assert [r["name"] for r in ge.CMH_RULES] == ["k_cmhE", "k_cmh_support", "k_cmh_fill"]
    for name in ("k_cmhE", "k_cmh_support", "k_cmh_fill", "k_cmh_exact", "k_cmh_odds_exact"):
        assert len([k for k in res if name in k]) == 1, name
    ge.check_kernel_resources(res, ge.RESOURCE_RULES + ge.CMH_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES +
                              ge.CMH_HOMOG_RULES)
