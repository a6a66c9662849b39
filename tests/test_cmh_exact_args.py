"""--cmh-exact: the argument checks on the command line (they exit before the engine is touched) and in
Setup_results (the same rules as ValueErrors), the place of the column and the resource rule of the kernel (the
declarations of the entry points: test_host_logic.py)."""
import os

import pytest

from args_cases import COLUMNS, good_strata_file as _strata_file, rule_of, run_refused as _run

FLAG, KW = "--cmh-exact", "cmh_exact"
NO_CMH = "Cannot use --cmh-exact without --cmh FILE. The exact test is taken over the strata of FILE"


def test_flag_parsing():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.cmh_exact is False
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--cmh", "s.csv", "--cmh-exact"])
    assert args.cmh_exact is True and args.cmh == "s.csv" and args.permute == 0
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--cmh", "s.csv", "--cmh-exact", "--cmh-fwer",
                                         "--cmh-fwer-stepdown", "--permute-fwer", "-e", "100"])
    assert args.cmh_exact and args.cmh_fwer and args.cmh_fwer_stepdown and args.permute_fwer


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    from scoary_amd import dist, methods as m
    path = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    no_pairwise = ("Cannot use --cmh-exact without --no_pairwise. The exact conditional test is a test of every gene "
                   "over the strata, beside Fisher's")
    assert run([FLAG]) == no_pairwise
    assert run([FLAG, "--cmh", path]).startswith("Cannot use --cmh without --no_pairwise")
    assert run(["--no_pairwise", FLAG]) == NO_CMH
    assert run(["--no_pairwise", FLAG, "-e", "100"]) == NO_CMH
    assert run(["--no_pairwise", FLAG, "-e", "100", "--permute-strata", path]) == NO_CMH
    assert run(["--no_pairwise", FLAG, "--cmh", path, "-e", "100", "--permute-early-abort"]) \
        .startswith("Cannot use --cmh together with --permute-early-abort")
    rule = rule_of(FLAG)
    assert list(m._broken_rules(rule, False, 0, False, (), cmh=False)) == [no_pairwise, NO_CMH]
    assert list(m._broken_rules(rule, True, 0, False, (), cmh=True)) == []         # no permutations needed
    assert list(m._broken_rules(rule, True, 100, False, (), cmh=True)) == []
    monkeypatch.setattr(dist, "world_rank", lambda: (2, 0))
    assert run(["--no_pairwise", FLAG, "--cmh", path]).startswith("Cannot use --cmh under more than one rank")
    assert list(m._broken_rules(rule, True, 0, False, (), cmh=True)) == \
        ["Cannot use --cmh-exact under more than one rank: %s" % rule.one_rank]
    assert list(m._broken_rules(rule, True, 0, False, None, cmh=True)) == \
        ["cmh_exact needs a single process: %s" % rule.one_rank]


def test_setup_results_raises_the_same_rules():
    from scoary_amd import methods as m
    for kw in ({}, {"permutations": 100}, {"permutations": 100, "strata": [0, 1]}):
        with pytest.raises(ValueError, match=r"cmh_exact needs cmh \(and its strata\)"):
            m.Setup_results({}, {}, False, cmh_exact=True, **kw)
    with pytest.raises(ValueError, match="cmh needs strata"):
        m.Setup_results({}, {}, False, cmh=True, cmh_exact=True)


def test_the_engine_refuses_the_exact_test_without_cmh():
    from scoary_amd.engine import AssociationEngine
    with pytest.raises(ValueError, match=r"cmh_exact=True needs cmh=True"):
        AssociationEngine.associate(None, None, None, None, cmh_exact=True)


def test_columns_are_in_file_order_and_the_rule_keeps_the_shape_of_its_row():
    from scoary_amd import methods as m
    assert m.OPTIONAL_COLUMNS == COLUMNS
    rule = rule_of(FLAG)
    assert rule is m.FLAG_RULES[len(m.FLAG_RULES) - 1]                      # checked after every other flag
    assert (rule.kw, rule.needs_permutations, rule.no_early_abort, rule.needs_cmh) == (KW, False, False, "cmh_exact")
    assert rule.one_rank == rule_of("--cmh").one_rank
    assert m.RULE_TEXT["cmh_exact"][0] % {"flag": FLAG} == NO_CMH


def test_kernel_compiled_to_its_resource_rule_and_the_cmh_kernels_kept_theirs():
    import json
    import __graft_entry__ as ge
    if not os.path.exists(ge.HIP_RESOURCES):
        ge.build()
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    assert any(s.endswith("scoary_cmh_exact.hip") for s in ge.HIP_SRCS)
    hit = [v for k, v in res.items() if "k_cmh_exact" in k]
    assert len(hit) == 1
    assert hit[0]["ScratchSize"] == 0 and hit[0]["VGPRs Spill"] == 0 and hit[0]["SGPRs Spill"] == 0
    (rule,) = ge.CMH_EXACT_RULES
    assert rule["name"] == "k_cmh_exact" and rule["cap"][1] <= 64 and hit[0]["VGPRs"] <= rule["cap"][1]
    for other in ge.CMH_RULES:                     # the new kernel is in none of the existing families
        assert other["name"] not in "k_cmh_exactE"
    ge.check_kernel_resources(res, ge.RESOURCE_RULES + ge.CMH_RULES + ge.CMH_EXACT_RULES)
