"""--categorical-fwer-stepdown through main(): the clonal two-lineage population of the generalized CMH test
(gcmh_spec's scenario with --categorical-fwer's genes and twenty more noise genes: the marker of a lineage is compared
with a family behind it), run with the flag, with both family-wise flags and with neither, with and without
--categorical-strata.  Westfall_Young_stepdown_p is the last column of the chi-square file and of the generalized CMH
file and holds the restatement's value (cat_sd_spec.py); it is never above Westfall_Young_p and strictly below it for
some gene; the lineage marker leads the chi-square family and is unremarkable inside the lineages; every other cell and
every other file is what the run without the flag writes."""
import csv
import io
import sys

import numpy as np
import pytest

import cat_sd_spec as sd
import cat_wy_spec as ws
import categorical_spec as cs
import gcmh_spec as gs
from test_gpu_cat_wy_cli import _write_table
from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
P, SEED = 60, 4242
FLAG, FWER = "--categorical-fwer-stepdown", "--categorical-fwer"
CHI, GCMH, BIN = "host.categorical.results.csv", "host.gcmh.results.csv", "bin.results.csv"


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("cat_sd_cli")
    genes, labels, strata = gs.clonal_scenario()
    rng = np.random.default_rng(9)
    genes = genes + [[int(rng.random() < f) for _ in strata] for f in (0.2, 0.5, 0.8, 0.35)]
    genes.append([1] * len(strata))                                                            # an untestable gene
    rng = np.random.default_rng(23)
    genes = genes + [[int(rng.random() < f) for _ in strata] for f in rng.uniform(0.1, 0.9, 20)]
    iso = ["i%03d" % i for i in range(len(labels))]
    _write_table(d / "g.csv", genes, iso)
    (d / "t.csv").write_text(",bin\n" + "".join("%s,%d\n" % (s, i % 2) for i, s in enumerate(iso)))
    (d / "c.csv").write_text("Name,host\n" + "".join("%s,%s\n" % x for x in zip(iso, labels)))
    (d / "s.csv").write_text("Isolate,Lineage\n" + "".join("%s,L%d\n" % x for x in zip(iso, strata)))
    common = ["-g", str(d / "g.csv"), "-t", str(d / "t.csv"), "--no_pairwise", "--seed", str(SEED), "-p", "1.0",
              "--categorical", str(d / "c.csv"), "-e", str(P)]
    strata_flag = ["--categorical-strata", str(d / "s.csv")]
    return dict(genes=genes, labels=labels, strata=strata, dir=d, common=common,
                plain=run_cli(common + strata_flag, d / "out_plain"),
                fwer=run_cli(common + strata_flag + [FWER], d / "out_fwer"),
                sd=run_cli(common + strata_flag + [FLAG], d / "out_sd"),
                both=run_cli(common + strata_flag + [FWER, FLAG], d / "out_both"),
                sd_chi=run_cli(common + [FLAG], d / "out_sd_chi"))


def _split(text):
    rows = list(csv.reader(io.StringIO(text)))
    return rows[0], rows[1:]


def test_the_column_order_and_everything_else_is_what_the_other_runs_write(data):
    for run in ("plain", "fwer", "sd", "both"):
        assert sorted(data[run]) == [BIN, CHI, GCMH], run
        assert data[run][BIN] == data["plain"][BIN]                      # every other file: byte for byte
    assert sorted(data["sd_chi"]) == [BIN, CHI] and data["sd_chi"][BIN] == data["plain"][BIN]
    assert data["sd_chi"][CHI] == data["sd"][CHI]                        # the strata change nothing in the chi-square file
    for name in (CHI, GCMH):
        base, fwer = data["plain"][name].splitlines(), data["fwer"][name].splitlines()
        alone, both = data["sd"][name].splitlines(), data["both"][name].splitlines()
        assert len(base) == len(alone) == len(both) == 28                # 27 testable genes
        assert base[0].endswith('"Empirical_p"')
        # the flag alone: Westfall_Young_stepdown_p and no Westfall_Young_p
        assert alone[0] == base[0] + ',"Westfall_Young_stepdown_p"' and "Westfall_Young_p" not in alone[0]
        assert [l.rsplit(",", 1)[0] for l in alone] == base              # every other cell: the run without the flag
        # both flags: the step-down column is the last, behind Westfall_Young_p
        assert both[0] == base[0] + ',"Westfall_Young_p","Westfall_Young_stepdown_p"'
        assert [l.rsplit(",", 1)[0] for l in both] == fwer
        assert [l.rsplit(",", 1)[1] for l in both] == [l.rsplit(",", 1)[1] for l in alone]


def test_the_step_down_p_is_the_restatements_and_gains_on_the_single_step_one(data):
    from scoary_amd import methods as m
    genes, strata = np.array(data["genes"]), np.array(data["strata"])
    classes, codes = cs.codes_of(data["labels"])
    assert classes == ["cattle", "human", "pig"]
    fmt = lambda r: m._fmt((int(r) + 1.0) / (P + 1.0))                   # noqa: E731
    # chi-square: S20's shuffle
    rows = np.array([cs.perm_row(SEED, 0, pi, codes) for pi in range(P)])
    tr = sd.chi2_trait(genes, np.array(codes), rows)
    out = sd.stepdown(tr["cells"], tr["thr"])
    rf = ws.r_fwer(ws.maxs(tr["cells"]), tr["thr"])
    head, lines = _split(data["both"][CHI])
    assert head[-3:] == ["Empirical_p", "Westfall_Young_p", "Westfall_Young_stepdown_p"] and len(lines) == 27
    below = 0
    for line in lines:
        g = int(line[0][1:])
        assert line[-3:] == [fmt(tr["r"][g]), fmt(rf[g]), fmt(out["r_sd"][g])], g
        assert float(line[-3]) <= float(line[-1]) <= float(line[-2])
        below += float(line[-1]) < float(line[-2])
    assert "g007" not in [line[0] for line in lines] and out["r_sd"][7] == P       # the untestable gene: no row
    # the lineage marker keeps the smallest family-wise p there is, in both columns ..
    marker = next(line for line in lines if line[0] == "g000")
    assert marker[-2] == marker[-1] == fmt(0) == min((line[-1] for line in lines), key=float)
    # .. and other genes, no longer compared with the marker's permuted cells, gain
    assert below >= 1 and below == int((out["r_sd"] < rf).sum())
    # generalized CMH: S21's shuffle within the lineages
    qrows = np.array([gs.perm_row(SEED, 0, pi, codes, strata.tolist(), 2) for pi in range(P)])
    tq = sd.gcmh_trait(genes, np.array(codes), strata, 2, qrows)
    oq = sd.stepdown(tq["cells"], tq["thr"])
    rq = ws.r_fwer(ws.maxs(tq["cells"]), tq["thr"])
    head, lines = _split(data["both"][GCMH])
    assert head[-3:] == ["Empirical_p", "Westfall_Young_p", "Westfall_Young_stepdown_p"] and len(lines) == 27
    for line in lines:
        g = int(line[0][1:])
        assert line[-3:] == [fmt(tq["r"][g]), fmt(rq[g]), fmt(oq["r_sd"][g])], g
        assert float(line[-3]) <= float(line[-1]) <= float(line[-2])
    # inside the lineages the marker is unremarkable: 1.0 in both columns; the gene that follows the label leads
    marker = next(line for line in lines if line[0] == "g000")
    assert marker[-2:] == ["1.0", "1.0"]
    within = next(line for line in lines if line[0] == "g001")
    assert within[-2:] == [fmt(0), fmt(0)]
    assert (oq["r_sd"] < rq).any()


def test_the_refusals_exit_with_their_messages(data, monkeypatch):
    from scoary_amd import methods as m
    base = [a for a in data["common"] if a not in ("-e", str(P))]
    for argv, text in ((base + [FLAG], m.CAT_SD_TEXT["permute"]),
                       (base[:base.index("--categorical")] + ["-e", str(P), FLAG], m.CAT_SD_TEXT["categorical"])):
        monkeypatch.setattr(sys, "argv", ["scoary"] + argv + ["-o", str(data["dir"] / "out_refused"), "--no-time"])
        with pytest.raises(SystemExit) as e:
            m.main()
        assert e.value.code == text
