"""--covariates-spa and --covariates-spa-cutoff: the refusals on the command line (they exit before the engine is
touched) and in Score_results (the same rules as ValueErrors), the help text, the four last columns as the writer
lays them out, and what spec S25 adds to the binding, the header and the build."""
import os
import re

import numpy as np
import pytest

from args_cases import run_refused as _run, strains as _strains

SPA, CUT = "--covariates-spa", "--covariates-spa-cutoff"
NEEDS = ("Cannot use --covariates-spa without --covariates. The saddlepoint p corrects the logistic score test of "
         "--covariates FILE")
ALONE = "Cannot use --covariates-spa-cutoff without --covariates-spa"
CUTOFF = ("Cannot use --covariates-spa-cutoff %s: the cutoff is a finite number of at least 0.1 standard deviations "
          "(default 2.0)")


def _cov(exampledir, tmp_path):
    path = os.path.join(str(tmp_path), "cov.csv")
    with open(path, "w") as f:
        f.write("Name,pc1,pc2\n" + "".join("%s,%d.5,%d.25\n" % (s, (3 * i) % 7, (5 * i) % 11)
                                         for i, s in enumerate(_strains(exampledir))))
    return path


def test_flags_are_off_by_default_and_parse():
    from scoary_amd import methods as m
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv"])
    assert args.covariates_spa is False and args.covariates_spa_cutoff is None
    args, _cut = m.ScoaryArgumentParser(["-g", "g.csv", "-t", "t.csv", "--no_pairwise", "--covariates", "c.csv", SPA,
                                         CUT, "3.5"])
    assert args.covariates_spa is True and args.covariates_spa_cutoff == 3.5
    assert (m.SCORE_SPA_CUTOFF, m.SCORE_SPA_MIN_CUTOFF) == (2.0, 0.1)


def test_command_line_refusals(exampledir, tmp_path, monkeypatch):
    c = _cov(exampledir, tmp_path)
    run = lambda argv: _run(argv, exampledir, tmp_path, monkeypatch)          # noqa: E731
    assert run(["--no_pairwise", SPA]) == NEEDS
    assert run([SPA]) == NEEDS
    assert run(["--no_pairwise", SPA, CUT, "0.05"]) == NEEDS                   # in this order
    assert run(["--no_pairwise", "--covariates", c, CUT, "3"]) == ALONE
    assert run(["--no_pairwise", CUT, "3"]) == ALONE
    for text, shown in (("0.0999", "0.0999"), ("0", "0.0"), ("-2", "-2.0"), ("nan", "nan"), ("inf", "inf")):
        assert run(["--no_pairwise", "--covariates", c, SPA, CUT, text]) == CUTOFF % shown
    # the rules of --covariates itself come behind: the saddlepoint flags change none of them
    assert run(["--covariates", c, SPA]).startswith("Cannot use --covariates without --no_pairwise")


def test_a_cutoff_that_is_no_number_is_the_parsers_error(exampledir, tmp_path, monkeypatch, capsys):
    import sys
    from scoary_amd import methods as m
    monkeypatch.setattr(sys, "argv", ["scoary", "-g", "g.csv", "-t", "t.csv", "--no_pairwise", "--covariates",
                                      _cov(exampledir, tmp_path), SPA, CUT, "two"])
    with pytest.raises(SystemExit) as e:
        m.main()
    assert e.value.code == 2 and "--covariates-spa-cutoff: invalid float value: 'two'" in capsys.readouterr().err


def test_the_library_raises_the_same_rules(monkeypatch):
    from scoary_amd import methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    values, cov = np.array([[0.0, 1.0, np.nan]]), np.array([[0.5, 1.5, 2.5]])
    for kw, text in ((dict(spa_cutoff=3.0), "a saddlepoint cutoff without the saddlepoint p"),
                     (dict(spa=True, spa_cutoff=0.05), "the saddlepoint cutoff 0.05 is not a finite number of at least"),
                     (dict(spa=True, spa_cutoff=float("nan")), "the saddlepoint cutoff nan is not a finite number"),
                     (dict(spa=True, kind="linear"), "the saddlepoint p belongs to the logistic score test"),
                     (dict(spa=True, no_pairwise=False), "covariates need no_pairwise")):
        with pytest.raises(ValueError, match=text):
            m.Score_results(None, ["x"], values, ["pc1"], cov, **kw)
    assert list(m.SCORE_SPA_TEXT) == ["covariates", "kind", "alone", "cutoff"]
    assert m.SCORE_SPA_TEXT["covariates"][0] == NEEDS and m.SCORE_SPA_TEXT["alone"][0] == ALONE
    assert m.SCORE_SPA_TEXT["cutoff"][0] % ("0.05", 0.1, 2.0) == CUTOFF % "0.05"
    assert list(m._score_spa_refusals(True, True, None)) == [] == list(m._score_spa_refusals(False, False, None))
    assert list(m._score_spa_refusals(True, True, 0.1)) == []


def test_help_text_says_what_the_columns_are_and_what_max_hits_cuts_by(capsys):
    from scoary_amd import methods as m
    with pytest.raises(SystemExit):
        m.ScoaryArgumentParser(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for piece in ("--covariates-spa ", "--covariates-spa-cutoff X", "SPA_p", "SPA_Bonferroni_p", "SPA_Benjamini_H_p",
                  "SPA_status", "--max_hits still cuts by Score_p", "the linear files are untouched",
                  "default 2.0, at least 0.1"):
        assert piece in text, piece


def test_the_writer_puts_the_four_columns_last_and_changes_nothing_else(tmp_path):
    """StoreScoreResults on a result by hand, with and without the saddlepoint keys: the file with them, less its four
    last columns, is the file without; the cells are SPA_p, bonferroni_bh over the same genes, and the status."""
    from scoary_amd import methods as m
    G = 6
    table = {"ids": ["g%d" % g for g in range(G)]}
    res = dict(n=40, kind="logistic", m=np.array([3, 9, 20, 0, 7, 5]), beta=np.linspace(-1, 1, G),
               se=np.full(G, 0.5), stat=np.array([9.0, 0.2, 4.5, 0.0, 1.0, 6.0]),
               p=np.array([2.7e-3, 0.65, 3.4e-2, 1.0, 0.32, 1.4e-2]),
               testable=np.array([True, True, True, False, True, True]))
    spa = dict(res, spa_p=np.array([4.1e-2, 0.65, 3.0e-2, 1.0, 0.32, 1.4e-2]),
               spa_status=np.array([1, 0, 1, 0, 0, 2], dtype=np.int32))

    class Table:
        ids = table["ids"]
        nugn = [""] * G
        annotation = [""] * G
    files = {}
    for key, r, hits in (("plain", res, None), ("spa", spa, None), ("plain3", res, 3), ("spa3", spa, 3)):
        out = os.path.join(str(tmp_path), key) + os.sep
        os.mkdir(out)
        orig = m._as_table
        m._as_table = lambda _g: Table
        try:
            (name,) = m.StoreScoreResults({"trait": r}, None, hits, out)
        finally:
            m._as_table = orig
        with open(name) as f:
            files[key] = [line.rstrip("\n").split(",") for line in f]
    for plain, with_spa in (("plain", "spa"), ("plain3", "spa3")):
        assert [row[:-4] for row in files[with_spa]] == files[plain]
    assert files["spa"][0][-4:] == ['"%s"' % c for c in m.SCORE_SPA_COLUMNS]
    assert m.SCORE_SPA_COLUMNS == ("SPA_p", "SPA_Bonferroni_p", "SPA_Benjamini_H_p", "SPA_status")
    assert len(files["spa"]) == 6 and len(files["spa3"]) == 4                   # max_hits cuts by Score_p
    idx = np.flatnonzero(spa["testable"])
    bonf, bh = m.bonferroni_bh(spa["spa_p"][idx], len(idx))
    order = np.argsort(spa["p"][idx], kind="stable")
    for row, k in zip(files["spa"][1:], order):
        g = idx[k]
        assert row[0] == '"g%d"' % g
        assert row[-4:] == ['"%s"' % m._fmt(x) for x in (spa["spa_p"][g], bonf[k], bh[k], int(spa["spa_status"][g]))]


def test_the_feature_is_in_the_binding_the_header_and_the_build():
    import __graft_entry__ as ge
    from scoary_amd import _abi
    assert _abi.ABI_VERSION == 11
    with open(_abi.HEADER_PATH) as f:
        header = f.read()
    assert "spec S25" in header
    for name in ("scoary_score_spa_max_isolates", "scoary_score_spa_scratch_bytes", "scoary_score_spa"):
        assert name in _abi.SIGNATURES
        (proto,) = re.findall(r"\n(?:int|int64_t) %s\(([^;]*)\);" % name, header)
        count = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert count == len(_abi.SIGNATURES[name][1]), name
    import ctypes
    res, args = _abi.SIGNATURES["scoary_score_spa"]
    assert args[15] is ctypes.c_double and args.count(ctypes.c_double) == 1       # cutoff2, as the header has it
    (proto,) = re.findall(r"\nint scoary_score_spa\(([^;]*)\);", header)
    assert [a.split()[0] == "double" and "*" not in a for a in proto.split(",")].index(True) == 15
    if os.path.exists(_abi.LIB_PATH):
        lib = ctypes.CDLL(_abi.LIB_PATH)
        lib.scoary_score_spa_max_isolates.restype = ctypes.c_int64
        lib.scoary_score_spa_scratch_bytes.restype = ctypes.c_int64
        lib.scoary_score_spa_scratch_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
        assert lib.scoary_score_spa_max_isolates() >= 16320 and lib.scoary_abi_version() == 11
        assert lib.scoary_score_spa_scratch_bytes(50000, 10) >= 256 + 4 * 500000
        assert lib.scoary_score_spa_scratch_bytes(0, 10) == 0 == lib.scoary_score_spa_scratch_bytes(1 << 30, 4)
        assert hasattr(lib, "scoary_score_spa")
    assert any(s.endswith("scoary_score_spa.hip") for s in ge.HIP_SRCS)
    rules = {r["name"]: r for r in ge.SCORE_SPA_RULES}
    assert sorted(rules) == ["k_score_spa", "k_spa_finish", "k_spa_select", "k_spa_sums"]
    assert rules["k_score_spa"]["count"] == 9 == rules["k_spa_sums"]["count"]
    assert rules["k_spa_select"]["count"] == 1 == rules["k_spa_finish"]["count"]
    assert all(r["cap"] and r["scratch"] == 0 and r["sgpr_spills"] == 0 for r in rules.values())
    names = ["_ZN12_GLOBAL__N_111k_score_spaILi%dEEEvNS_7SpaArgsE" % q for q in range(1, 10)]
    names += ["_ZN12_GLOBAL__N_110k_spa_sumsILi%dEEEvNS_7SpaArgsE" % q for q in range(1, 10)]
    names += ["_ZN12_GLOBAL__N_112k_spa_selectENS_7SpaArgsEl", "_ZN12_GLOBAL__N_112k_spa_finishENS_7SpaArgsE"]
    ok = {n: {"VGPRs": 20, "AGPRs": 0, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0} for n in names}
    ge.check_kernel_resources(ok, ge.SCORE_SPA_RULES)
    for field, what in (("ScratchSize", "scratch 8"), ("SGPRs Spill", "SGPR spills 8"), ("VGPRs Spill", "VGPR spills 8")):
        for victim in (names[4], names[12], names[18], names[19]):
            bad = {k: dict(v, **({field: 8} if k == victim else {})) for k, v in ok.items()}
            with pytest.raises(RuntimeError, match=what):
                ge.check_kernel_resources(bad, ge.SCORE_SPA_RULES)
    cap = rules["k_score_spa"]["cap"][1]
    with pytest.raises(RuntimeError, match="%d VGPRs > %d" % (cap + 1, cap)):
        ge.check_kernel_resources(dict(ok, **{names[0]: dict(ok[names[0]], VGPRs=cap + 1)}), ge.SCORE_SPA_RULES)
    with pytest.raises(RuntimeError, match="expected 9 k_score_spa instances, compiler reported 8"):
        ge.check_kernel_resources({n: ok[n] for n in names[1:]}, ge.SCORE_SPA_RULES)
    every = (ge.RESOURCE_RULES + ge.LABELS_BFRAG_RULES + ge.CMH_RULES + ge.CMH_EXACT_RULES + ge.CMH_EXACT_ODDS_RULES +
             ge.CMH_HOMOG_RULES + ge.FISHER_CHAINS_RULES + ge.RANKSUM_RULES + ge.VANELTEREN_RULES + ge.RANK_WY_RULES +
             ge.RANK_SD_RULES + ge.RANK_SHIFT_RULES + ge.CATEGORICAL_RULES + ge.GCMH_RULES + ge.CAT_WY_RULES +
             ge.CAT_SD_RULES + ge.SCORE_RULES)
    for other in every:                               # the new names are in no other family, and in one of their own
        assert not any(other["name"] in n and not (other["exclude"] and other["exclude"] in n) for n in names)
    for n in names:
        assert sum(r["name"] in n for r in ge.SCORE_SPA_RULES) == 1, n
    if os.path.exists(ge.HIP_RESOURCES):
        import json
        with open(ge.HIP_RESOURCES) as f:
            ge.check_kernel_resources(json.load(f), ge.SCORE_SPA_RULES)
