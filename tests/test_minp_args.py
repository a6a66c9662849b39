"""--permute-fwer: the argument checks (host only -- they exit before the engine is touched; the declarations of
the entry points: test_host_logic.py)."""
import pytest

from args_cases import run_refused as _run


@pytest.mark.parametrize("argv,message", [
    (["--permute-fwer", "-e", "100"], "Cannot use --permute-fwer without --no_pairwise"),
    (["--permute-fwer", "--no_pairwise"], "Cannot use --permute-fwer without performing permutations"),
    (["--permute-fwer", "--no_pairwise", "-e", "5"], "Cannot use --permute-fwer without performing permutations"),
    (["--permute-fwer", "--no_pairwise", "-e", "100", "--permute-early-abort"],
     "Cannot use --permute-fwer together with --permute-early-abort"),
])
def test_permute_fwer_refusals(exampledir, tmp_path, monkeypatch, argv, message):
    code = _run(argv, exampledir, tmp_path, monkeypatch)
    assert isinstance(code, str) and code.startswith(message), code


def test_flag_is_off_by_default():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.permute_fwer is False
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--permute-fwer"])
    assert args.permute_fwer is True


def test_setup_results_refuses_fwer_without_permutations():
    from scoary_amd import methods as m
    with pytest.raises(ValueError):
        m.Setup_results({}, {}, False, permutations=0, fwer=True)
    with pytest.raises(ValueError):
        m.Setup_results({}, {}, False, permutations=100, early_abort=True, fwer=True)
