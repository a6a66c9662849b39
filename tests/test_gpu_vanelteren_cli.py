"""--quantitative-strata FILE through main(): the reference's exampledata with a small quantitative file and a strata
file, --permute 100, run with the flag and without it -- the rank-sum files and every ordinary result file byte for
byte the same in both runs, and every cell of the .vanelteren.results.csv files the restatement's value
(vanelteren_spec.py) as the writer formats it."""
import csv
import io
import os

import numpy as np
import pytest

import vanelteren_spec as ve
from conftest import golden_text, read_dense
from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
P, SEED = 100, 4242
COLUMNS = ["Gene", "Non-unique Gene name", "Annotation", "Number_with_gene", "Number_without_gene", "Van_Elteren_AUC",
           "Van_Elteren_p", "Bonferroni_p", "Benjamini_H_p", "Empirical_p"]


@pytest.fixture(scope="module")
def data(exampledir, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    d = tmp_path_factory.mktemp("vanelteren_cli")
    ids, strains, genes, _names, _traits = read_dense(golden_text("exampledata/Gene_presence_absence.csv.gz"),
                                                      golden_text("exampledata/Tetracycline_resistance.csv.gz"))
    N = len(strains)
    rng = np.random.default_rng(21)
    labels = ["clade %d" % ((i * 5 // N) % 4) if i % 13 else "solo" for i in range(N)]     # five strata, uneven
    (d / "strata.csv").write_text("Isolate,Lineage\n" + "".join("%s,%s\n" % kv for kv in zip(strains, labels)))
    mic = np.round(np.exp2(rng.integers(-3, 4, N).astype(float)), 3)                       # MIC-like: heavy ties
    mic += np.asarray([int(lab[-1]) if lab != "solo" else 9 for lab in labels]) * 8.0      # the lineages differ
    growth = rng.standard_normal(N)
    vals = np.stack([mic, growth])
    vals[0, 4::17] = np.nan
    vals[1, 2] = np.nan
    (d / "q.csv").write_text("Name,mic,growth\n" + "".join(
        "%s,%s,%s\n" % (strains[i], "NA" if np.isnan(vals[0, i]) else repr(float(vals[0, i])),
                        "NA" if np.isnan(vals[1, i]) else repr(float(vals[1, i]))) for i in range(N)))
    common = ["-g", os.path.join(exampledir, "Gene_presence_absence.csv"),
              "-t", os.path.join(exampledir, "Tetracycline_resistance.csv"), "--no_pairwise", "-e", str(P),
              "--seed", str(SEED), "-p", "1.0", "--quantitative", str(d / "q.csv")]
    with_s = run_cli(common + ["--quantitative-strata", str(d / "strata.csv")], d / "out_s")
    without = run_cli(common, d / "out_plain")
    index = {}
    st = [index.setdefault(lab, len(index)) for lab in labels]                            # by first appearance
    return dict(ids=ids, genes=genes, vals=vals, st=st, S=len(index), with_s=with_s, without=without, dir=d)


def test_every_other_result_file_is_byte_identical(data):
    assert sorted(data["without"]) == ["Bogus_trait.results.csv", "Tetracycline_resistance.results.csv",
                                       "growth.ranksum.results.csv", "mic.ranksum.results.csv"]
    assert sorted(data["with_s"]) == sorted(list(data["without"]) + ["growth.vanelteren.results.csv",
                                                                     "mic.vanelteren.results.csv"])
    for name, text in data["without"].items():
        assert data["with_s"][name] == text, name
        assert len(text.splitlines()) > 10


def test_van_elteren_files_hold_the_restatements_values(data):
    from scoary_amd import methods as m
    genes, G = data["genes"], len(data["ids"])
    for t, name in enumerate(("mic", "growth")):
        text = data["with_s"][name + ".vanelteren.results.csv"]
        assert all(line.startswith('"') and line.endswith('"') for line in text.splitlines())
        rows = list(csv.reader(io.StringIO(text)))
        assert rows[0] == COLUMNS
        pl = ve.plan([float(v) for v in data["vals"][t]], data["st"], data["S"])
        n = sum(pl["n"])
        stats = []
        for g in range(G):
            D, ms = ve.statistic(genes[g], pl)
            stats.append((D, sum(ms)) + ve.tail(D, ms, pl))          # D, m, testable, var, den, auc, p
        testable = [g for g in range(G) if stats[g][2]]
        assert 10 < len(testable) < G and len(rows) - 1 == len(testable)
        order = sorted(testable, key=lambda g: (stats[g][6], g))     # ascending p, ties in file order
        assert [row[0] for row in rows[1:]] == [data["ids"][g] for g in order]
        p = np.asarray([stats[g][6] for g in testable])
        bonf, bh = m.bonferroni_bh(p, len(testable))
        want_rows = [ve.perm_row(SEED, t, pi, pl) for pi in range(P)]
        # #{pi : |D_pi| >= |D_obs|}; the sums are integers below 2^53, so the float64 product is exact
        d_perm = genes[testable].astype(np.float64) @ np.asarray(want_rows, dtype=np.float64).T
        r = (np.abs(d_perm) >= np.abs(np.asarray([stats[g][0] for g in testable], dtype=np.float64))[:, None]).sum(1)
        where, same = {g: k for k, g in enumerate(testable)}, 0
        for row, g in zip(rows[1:], order):
            k = where[g]
            D, mm, _ok, _var, _den, auc, pv = stats[g]
            assert row[3:6] == [m._fmt(mm), m._fmt(n - mm), m._fmt(auc)], (name, g)
            assert row[9] == m._fmt((r[k] + 1.0) / (P + 1.0)), (name, g)
            # p is the device's erfc against math.erfc: the three cells that hold it are repr() of a double within
            # S16's bar on p, 1e-10 relative, of the restatement's; every other cell is the restatement's string
            for cell, want in zip(row[6:9], (pv, bonf[k], bh[k])):
                assert cell == repr(float(cell)) and abs(float(cell) - want) <= 1e-10 * want, (name, g)
            same += row[6:9] == [m._fmt(pv), m._fmt(bonf[k]), m._fmt(bh[k])]
        print("%s: %d of %d rows have the restatement's p cells to the last digit" % (name, same, len(order)))
    log = open(os.path.join(str(data["dir"] / "out_s"), "scoary.log")).read()
    assert "Van Elteren test of mic: %d isolates with a value in %d strata" % (
        int((~np.isnan(data["vals"][0])).sum()), data["S"]) in log
