"""--cmh-fwer / --cmh-fwer-stepdown: the argument checks on the command line (they exit before the engine is touched)
and in Setup_results (the same rules as ValueErrors), the place of the two columns and the build's report on the
table kernels (the declarations of the entry points: test_host_logic.py)."""
import os
import re

import pytest

from args_cases import COLUMNS, good_strata_file as _strata_file, rule_of, run_refused as _run

FLAGS = (("--cmh-fwer", "cmh_fwer"), ("--cmh-fwer-stepdown", "cmh_fwer_stepdown"))


@pytest.mark.parametrize("flag,kw", FLAGS)
def test_command_line_refusals(exampledir, tmp_path, monkeypatch, flag, kw):
    path = _strata_file(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    from scoary_amd import methods as m
    rule = rule_of(flag)
    no_pairwise = ("Cannot use %s without --no_pairwise. The Westfall-Young minima are taken over the "
                   "Cochran-Mantel-Haenszel statistic of every gene" % flag)
    early_abort = ("Cannot use %s together with --permute-early-abort. Every gene has to see every permutation"
                   % flag)
    assert run([flag, "-e", "100"]) == no_pairwise
    # (with --cmh FILE in the same faulty run, the row of --cmh comes first and reports the same rule of its own)
    assert run([flag, "--cmh", path, "-e", "100"]).startswith("Cannot use --cmh without --no_pairwise")
    for argv in (["--no_pairwise", flag, "--cmh", path], ["--no_pairwise", flag, "--cmh", path, "-e", "9"]):
        code = run(argv)
        assert code == ("Cannot use %s without performing permutations. Use '--permute X' where X is a number equal "
                        "to or larger than 10" % flag), code
    assert run(["--no_pairwise", flag, "-e", "100", "--permute-early-abort"]) == early_abort
    assert run(["--no_pairwise", flag, "--cmh", path, "-e", "100", "--permute-early-abort"]) \
        .startswith("Cannot use --cmh together with --permute-early-abort")
    assert list(m._broken_rules(rule, False, 100, True, (), cmh=True)) == [no_pairwise, early_abort]
    for argv in (["--no_pairwise", flag, "-e", "100"], ["--no_pairwise", flag, "-e", "100", "--permute-strata", path]):
        code = run(argv)
        assert code == ("Cannot use %s without --cmh FILE. The minima are taken over the statistic of the "
                        "Cochran-Mantel-Haenszel test over the strata of FILE" % flag), code


@pytest.mark.parametrize("flag,kw", FLAGS)
def test_rank_rule(exampledir, tmp_path, monkeypatch, flag, kw):
    from scoary_amd import dist
    path = _strata_file(exampledir, tmp_path)
    monkeypatch.setattr(dist, "world_rank", lambda: (2, 0))
    code = _run(["--no_pairwise", flag, "--cmh", path, "-e", "100"], exampledir, tmp_path, monkeypatch)
    # --cmh's own rank rule is met first (its row comes first); alone, the new flag's rule has the row's reason
    assert code.startswith("Cannot use --cmh under more than one rank"), code
    from scoary_amd import methods as m
    rule = rule_of(flag)
    why = {"--cmh-fwer": rule_of("--cmh"), "--cmh-fwer-stepdown": rule_of("--permute-fwer-stepdown")}[flag].one_rank
    assert why and list(m._broken_rules(rule, True, 100, False, (), cmh=True)) == \
        ["Cannot use %s under more than one rank: %s" % (flag, why)]
    assert list(m._broken_rules(rule, True, 100, False, None, cmh=True)) == \
        ["%s needs a single process: %s" % (kw, why)]


@pytest.mark.parametrize("flag,kw", FLAGS)
def test_setup_results_raises_the_same_rules(flag, kw):
    from scoary_amd import methods as m
    with pytest.raises(ValueError, match="%s needs the Fisher-statistic permutations of --no_pairwise "
                                         r"\(permutations >= 10\)" % kw):
        m.Setup_results({}, {}, False, strata=[0, 1], cmh=True, **{kw: True})
    with pytest.raises(ValueError, match="%s excludes early_abort" % kw):
        m.Setup_results({}, {}, False, permutations=100, early_abort=True, strata=[0, 1], **{kw: True})
    with pytest.raises(ValueError, match=r"%s needs cmh \(and its strata\)" % kw):
        m.Setup_results({}, {}, False, permutations=100, **{kw: True})
    with pytest.raises(ValueError, match=r"%s needs cmh \(and its strata\)" % kw):
        m.Setup_results({}, {}, False, permutations=100, strata=[0, 1], **{kw: True})


def test_flags_are_off_by_default_and_may_all_be_combined():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.cmh_fwer is False and args.cmh_fwer_stepdown is False
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--cmh", "s.csv", "--cmh-fwer",
                                         "--cmh-fwer-stepdown", "--permute-fwer", "--permute-fwer-stepdown"])
    assert args.cmh_fwer and args.cmh_fwer_stepdown and args.permute_fwer and args.permute_fwer_stepdown
    for rule in m.FLAG_RULES:                                   # none of the four excludes another
        assert list(m._broken_rules(rule, True, 100, False, (), cmh=True)) == []


def test_columns_and_rules_are_in_their_places():
    from scoary_amd import methods as m
    assert m.OPTIONAL_COLUMNS == COLUMNS
    at = COLUMNS.index(("CMH_empirical_p", "r_cmh", True))
    assert COLUMNS[at + 1:at + 3] == (("CMH_Westfall_Young_p", "r_cmh_fwer", True),
                                      ("CMH_Westfall_Young_stepdown_p", "r_cmh_fwer_sd", True))
    for flag, kw in FLAGS:
        rule = rule_of(flag)
        assert (rule.kw, rule.needs_permutations, rule.no_early_abort, rule.needs_cmh) == (kw, True, True, "cmh")
        assert rule.one_rank
    assert rule_of("--cmh-fwer").one_rank == rule_of("--cmh").one_rank
    assert rule_of("--cmh-fwer-stepdown").one_rank == rule_of("--permute-fwer-stepdown").one_rank
    assert [r.flag for r in m.FLAG_RULES if r.needs_cmh == "cmh"] == [flag for flag, _kw in FLAGS]


def test_table_kernels_compiled_without_scratch_or_spills_and_k_cmh_is_one_kernel_still():
    import json
    import __graft_entry__ as ge
    if not os.path.exists(ge.HIP_RESOURCES):
        ge.build()
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    for name in ("k_cmh_support", "k_cmh_fill"):
        hit = [v for k, v in res.items() if name in k]
        assert len(hit) == 1, name
        assert hit[0]["ScratchSize"] == 0 and hit[0]["VGPRs Spill"] == 0 and hit[0]["SGPRs Spill"] == 0
    assert len([k for k in res if re.search(r"\d+k_cmhE", k)]) == 1
    assert {rule["name"] for rule in ge.CMH_RULES} == {"k_cmhE", "k_cmh_support", "k_cmh_fill"}
    ge.check_kernel_resources(res, ge.RESOURCE_RULES + ge.CMH_RULES)
