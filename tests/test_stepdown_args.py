"""--permute-fwer-stepdown: the argument checks (host only -- they exit before the engine is touched; the declarations
of the step-down entry points: test_host_logic.py)."""
import pytest

from args_cases import run_refused as _run


@pytest.mark.parametrize("argv,message", [
    (["--permute-fwer-stepdown", "-e", "100"], "Cannot use --permute-fwer-stepdown without --no_pairwise"),
    (["--permute-fwer-stepdown", "--no_pairwise"],
     "Cannot use --permute-fwer-stepdown without performing permutations"),
    (["--permute-fwer-stepdown", "--no_pairwise", "-e", "5"],
     "Cannot use --permute-fwer-stepdown without performing permutations"),
    (["--permute-fwer-stepdown", "--no_pairwise", "-e", "100", "--permute-early-abort"],
     "Cannot use --permute-fwer-stepdown together with --permute-early-abort"),
])
def test_permute_fwer_stepdown_refusals(exampledir, tmp_path, monkeypatch, argv, message):
    code = _run(argv, exampledir, tmp_path, monkeypatch)
    assert isinstance(code, str) and code.startswith(message), code


def test_permute_fwer_stepdown_refuses_more_than_one_rank(exampledir, tmp_path, monkeypatch):
    from scoary_amd import dist
    monkeypatch.setattr(dist, "world_rank", lambda: (2, 0))
    code = _run(["--permute-fwer-stepdown", "--no_pairwise", "-e", "100"], exampledir, tmp_path, monkeypatch)
    assert isinstance(code, str) and code.startswith("Cannot use --permute-fwer-stepdown under more than one rank"), code
    assert "the successive minima run over all genes in one order; gene shards do not compose" in code


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.permute_fwer_stepdown is False
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--permute-fwer-stepdown"])
    assert args.permute_fwer_stepdown is True and args.permute_fwer is False


def test_setup_results_refuses_stepdown(monkeypatch):
    """The four conditions, before the engine is touched (no pairwise stage = no permutations reach Setup_results)."""
    from scoary_amd import dist, methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    with pytest.raises(ValueError):
        m.Setup_results({}, {}, False, permutations=0, fwer_stepdown=True)
    with pytest.raises(ValueError):
        m.Setup_results({}, {}, False, permutations=5, fwer_stepdown=True)
    with pytest.raises(ValueError):
        m.Setup_results({}, {}, False, permutations=100, early_abort=True, fwer_stepdown=True)
    monkeypatch.setattr(dist, "world_rank", lambda: (2, 0))
    with pytest.raises(ValueError, match="gene shards do not compose"):
        m.Setup_results({}, {}, False, permutations=100, fwer_stepdown=True)
