"""What the test_*_args.py files share: the runner of a command line that has to be refused before the engine is
touched, and the strata files of the example data."""
import os
import sys

import pytest

# what methods.OPTIONAL_COLUMNS has to be: the optional columns of a results file, in file order -- (name, key of
# the step's array, True = a count)
COLUMNS = (("Westfall_Young_p", "r_fwer", True), ("Westfall_Young_stepdown_p", "r_fwer_sd", True),
           ("CMH_p", "cmh_p", False), ("CMH_odds_ratio", "cmh_odds", False), ("CMH_empirical_p", "r_cmh", True),
           ("CMH_Westfall_Young_p", "r_cmh_fwer", True), ("CMH_Westfall_Young_stepdown_p", "r_cmh_fwer_sd", True),
           ("CMH_exact_p", "cmh_exact_p", False), ("CMH_exact_odds_ratio", "cmh_exact_odds", False),
           ("CMH_exact_odds_ratio_lower", "cmh_exact_odds_lower", False),
           ("CMH_exact_odds_ratio_upper", "cmh_exact_odds_upper", False))


def strains(exampledir):
    with open(os.path.join(exampledir, "Gene_presence_absence.csv")) as f:
        return f.readline().rstrip("\n").split(",")[14:]


def good_rows(exampledir, *more):
    """A row per isolate of the example data, in three strata; ``more``: further cells of every row."""
    return [(s, "L%d" % (i % 3)) + more for i, s in enumerate(strains(exampledir))]


def strata_file(tmp_path, rows, name="strata.csv", header="Isolate,Stratum"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(header + "\n")
        for r in rows:
            f.write(",".join(r) + "\n")
    return path


def good_strata_file(exampledir, tmp_path):
    return strata_file(tmp_path, good_rows(exampledir))


def run_refused(argv, exampledir, tmp_path, monkeypatch):
    """The exit message of ``scoary <example data> argv``: the run ends before the engine is started, leaves no results
    file and exits with a message, not a status."""
    from scoary_amd import methods as m

    def no_engine():
        raise AssertionError("the engine was started before the arguments were refused")
    monkeypatch.setattr(m, "get_engine", no_engine)
    monkeypatch.setenv("SCOARY_OVERLAP_STARTUP", "0")
    out = os.path.join(str(tmp_path), "out")
    monkeypatch.setattr(sys, "argv", ["scoary", "-g", os.path.join(exampledir, "Gene_presence_absence.csv"),
                                      "-t", os.path.join(exampledir, "Tetracycline_resistance.csv"),
                                      "-o", out, "--no-time"] + argv)
    with pytest.raises(SystemExit) as e:
        m.main()
    assert not [f for f in os.listdir(out) if f.endswith(".results.csv")]
    assert isinstance(e.value.code, str), e.value.code
    return e.value.code


def rule_of(flag):
    """The row of methods.FLAG_RULES of ``flag``."""
    from scoary_amd import methods as m
    (rule,) = [r for r in m.FLAG_RULES if r.flag == flag]
    return rule
