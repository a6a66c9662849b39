"""--cmh: the argument checks (host only -- they exit before the engine is touched) and the build's report on k_cmh
(the declarations of the entry points: test_host_logic.py)."""
import json
import os
import re
import sys

import pytest

from args_cases import good_rows as _good_rows, run_refused as _run, strains as _strains, strata_file as _strata_file


def test_refused_without_no_pairwise_and_with_early_abort(exampledir, tmp_path, monkeypatch):
    path = _strata_file(tmp_path, _good_rows(exampledir))
    assert _run(["--cmh", path], exampledir, tmp_path, monkeypatch).startswith("Cannot use --cmh without --no_pairwise")
    assert _run(["--cmh", path, "-e", "100"], exampledir, tmp_path, monkeypatch) \
        .startswith("Cannot use --cmh without --no_pairwise")
    assert _run(["--cmh", path, "--no_pairwise", "-e", "100", "--permute-early-abort"], exampledir, tmp_path,
                monkeypatch).startswith("Cannot use --cmh together with --permute-early-abort")


def test_refused_file_problems(exampledir, tmp_path, monkeypatch):
    good = _good_rows(exampledir)
    code = _run(["--no_pairwise", "--cmh", os.path.join(str(tmp_path), "nowhere.csv")], exampledir, tmp_path, monkeypatch)
    assert code.startswith("Could not find the strata file"), code
    code = _run(["--no_pairwise", "--cmh", _strata_file(tmp_path, good[:-1], "absent.csv")], exampledir, tmp_path,
                monkeypatch)
    assert "does not name a stratum for 1 of the analysed isolates" in code and good[-1][0] in code, code


def test_refused_with_another_permute_strata_file(exampledir, tmp_path, monkeypatch):
    good = _good_rows(exampledir)
    one, two = _strata_file(tmp_path, good, "one.csv"), _strata_file(tmp_path, good, "two.csv")
    code = _run(["--no_pairwise", "-e", "100", "--cmh", one, "--permute-strata", two], exampledir, tmp_path, monkeypatch)
    assert "name different strata files" in code and one in code and two in code, code
    code = _run(["--no_pairwise", "-e", "100", "--cmh", one, "--permute-strata", os.path.join(str(tmp_path), "no.csv")],
                exampledir, tmp_path, monkeypatch)
    assert "name different strata files" in code, code
    # the same file under another spelling is the same file: the run gets past the arguments, to the engine
    from scoary_amd import methods as m
    monkeypatch.setattr(m, "get_engine", lambda: (_ for _ in ()).throw(RuntimeError("engine reached")))
    monkeypatch.setenv("SCOARY_OVERLAP_STARTUP", "0")
    again = os.path.join(str(tmp_path), ".", "one.csv")
    monkeypatch.setattr(sys, "argv", ["scoary", "-g", os.path.join(exampledir, "Gene_presence_absence.csv"),
                                      "-t", os.path.join(exampledir, "Tetracycline_resistance.csv"), "-o",
                                      os.path.join(str(tmp_path), "out2"), "--no-time", "--no_pairwise", "-e", "100",
                                      "--cmh", one, "--permute-strata", again])
    with pytest.raises((RuntimeError, SystemExit)) as e:
        m.main()
    assert "different strata files" not in str(e.value)


def test_refused_above_the_strata_limits(exampledir, tmp_path, monkeypatch):
    from scoary_amd import _abi
    own = [(s, "own%d" % i) for i, s in enumerate(_strains(exampledir))]
    path = _strata_file(tmp_path, own, "own.csv")
    monkeypatch.setattr(_abi, "PERM_MAX_STRATA", len(own) - 1)
    code = _run(["--no_pairwise", "--cmh", path], exampledir, tmp_path, monkeypatch)
    assert "names %d strata" % len(own) in code and "--cmh takes at most %d" % (len(own) - 1) in code, code
    monkeypatch.setattr(_abi, "PERM_MAX_STRATA", 1024)
    monkeypatch.setattr(_abi, "PERM_STRATA_MAX_ISOLATES", len(own) - 1)
    code = _run(["--no_pairwise", "--cmh", path], exampledir, tmp_path, monkeypatch)
    assert code.startswith("--cmh takes at most %d isolates" % (len(own) - 1)), code


def test_flag_is_off_by_default_and_setup_results_refuses_cmh_without_strata():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.cmh is None
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--cmh", "s.csv"])
    assert args.cmh == "s.csv"
    with pytest.raises(ValueError, match="strata"):
        m.Setup_results({}, {}, False, cmh=True)
    with pytest.raises(ValueError, match="early_abort"):
        m.Setup_results({}, {}, False, permutations=100, early_abort=True, strata=[0, 1], cmh=True)


def test_k_cmh_compiled_without_scratch_or_spills():
    """The accumulators of a trait chunk stay in registers (the build's kernel resource report)."""
    import __graft_entry__ as ge
    if not os.path.exists(ge.HIP_RESOURCES):
        ge.build()
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    hit = {k: v for k, v in res.items() if re.search(r"\d+k_cmhE", k)}
    assert len(hit) == 1, list(hit)
    r = next(iter(hit.values()))
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs"] <= 128
    lib = ge.HIP_SRCS
    assert any(s.endswith("scoary_cmh.hip") for s in lib)
