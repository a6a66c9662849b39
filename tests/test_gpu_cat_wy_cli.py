"""--categorical-fwer through main(): the clonal two-lineage population of the generalized CMH test (gcmh_spec's
scenario), run with the flag -- with and without --categorical-strata -- and without it: Westfall_Young_p is the last
column of the chi-square file and of the generalized CMH file and holds the restatement's value (cat_wy_spec.py), it is
never below Empirical_p, every other cell and every other file is byte for byte what the run without the flag writes,
and the refusals exit with their messages."""
import csv
import io
import sys

import numpy as np
import pytest

import cat_wy_spec as ws
import categorical_spec as cs
import gcmh_spec as gs
from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
P, SEED = 60, 4242
FLAG = "--categorical-fwer"
META = ["Gene", "Non-unique Gene name", "Annotation", "No. isolates", "No. sequences", "Avg sequences per isolate",
        "Genome Fragment", "Order within Fragment", "Accessory Fragment", "Accessory Order with Fragment", "QC",
        "Min group size nuc", "Max group size nuc", "Avg group size nuc"]


def _write_table(path, dense, iso):
    cells = np.where(np.asarray(dense, dtype=bool), "x", "")
    path.write_text(",".join(META + iso) + "\n" + "".join(
        "g%03d,nu%d,\"an, %d\",%s,%s\n" % (g, g, g, ",".join(["1"] * 11), ",".join(cells[g])) for g in range(len(cells))))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("cat_wy_cli")
    genes, labels, strata = gs.clonal_scenario()
    rng = np.random.default_rng(9)
    genes = genes + [[int(rng.random() < f) for _ in strata] for f in (0.2, 0.5, 0.8, 0.35)]      # more of the family
    genes.append([1] * len(strata))                                                            # and an untestable gene
    iso = ["i%03d" % i for i in range(len(labels))]
    _write_table(d / "g.csv", genes, iso)
    (d / "t.csv").write_text(",bin\n" + "".join("%s,%d\n" % (s, i % 2) for i, s in enumerate(iso)))
    (d / "c.csv").write_text("Name,host\n" + "".join("%s,%s\n" % x for x in zip(iso, labels)))
    (d / "s.csv").write_text("Isolate,Lineage\n" + "".join("%s,L%d\n" % x for x in zip(iso, strata)))
    common = ["-g", str(d / "g.csv"), "-t", str(d / "t.csv"), "--no_pairwise", "--seed", str(SEED), "-p", "1.0",
              "--categorical", str(d / "c.csv"), "-e", str(P)]
    strata_flag = ["--categorical-strata", str(d / "s.csv")]
    return dict(genes=genes, labels=labels, strata=strata, dir=d, common=common,
                plain=run_cli(common, d / "out_plain"), fwer=run_cli(common + [FLAG], d / "out_fwer"),
                plain_s=run_cli(common + strata_flag, d / "out_plain_s"),
                fwer_s=run_cli(common + strata_flag + [FLAG], d / "out_fwer_s"))


def _split(text):
    rows = list(csv.reader(io.StringIO(text)))
    return rows[0], rows[1:]


def test_the_column_is_the_last_and_everything_else_is_byte_identical(data):
    assert sorted(data["plain"]) == sorted(data["fwer"]) == ["bin.results.csv", "host.categorical.results.csv"]
    assert sorted(data["plain_s"]) == sorted(data["fwer_s"]) == ["bin.results.csv", "host.categorical.results.csv",
                                                                 "host.gcmh.results.csv"]
    assert data["fwer"]["bin.results.csv"] == data["plain"]["bin.results.csv"] == data["fwer_s"]["bin.results.csv"]
    assert data["plain_s"]["host.categorical.results.csv"] == data["plain"]["host.categorical.results.csv"]
    assert data["fwer_s"]["host.categorical.results.csv"] == data["fwer"]["host.categorical.results.csv"]
    for with_flag, without, name in ((data["fwer"], data["plain"], "host.categorical.results.csv"),
                                     (data["fwer_s"], data["plain_s"], "host.gcmh.results.csv")):
        lines, base = with_flag[name].splitlines(), without[name].splitlines()
        assert len(lines) == len(base) == 8                              # seven testable genes
        assert base[0].endswith('"Empirical_p"') and lines[0] == base[0] + ',"Westfall_Young_p"'
        assert [l.rsplit(",", 1)[0] for l in lines] == base              # one more cell a row, nothing else changes
        head, rows = _split(with_flag[name])
        for row in rows:
            assert float(row[-1]) >= float(row[head.index("Empirical_p")])
            assert 1.0 / (P + 1) <= float(row[-1]) <= 1.0


def test_westfall_young_p_is_the_restatements(data):
    from scoary_amd import methods as m
    genes, strata = data["genes"], data["strata"]
    classes, codes = cs.codes_of(data["labels"])
    assert classes == ["cattle", "human", "pig"]
    K = len(classes)
    # chi-square: S20's shuffle
    pr = ws.chi2_problem(genes, codes, K)
    rows = [cs.perm_row(SEED, 0, pi, codes) for pi in range(P)]
    rf = ws.r_fwer(ws.maxs(ws.chi2_cells(genes, rows, pr, K)), pr["thr"])
    r = [cs.r_count(g, rows, codes, K) for g in genes]
    head, lines = _split(data["fwer"]["host.categorical.results.csv"])
    assert head[-2:] == ["Empirical_p", "Westfall_Young_p"] and len(lines) == 7
    for line in lines:
        g = int(line[0][1:])
        assert line[-2:] == [m._fmt((r[g] + 1.0) / (P + 1.0)), m._fmt((int(rf[g]) + 1.0) / (P + 1.0))], g
    assert "g007" not in [line[0] for line in lines] and rf[7] == P    # the untestable gene: no row, r_fwer = P
    # the lineage marker is the family's maximum almost always: its family-wise p is the smallest there is
    assert rf[0] == r[0] == 0
    # generalized CMH: S21's shuffle within the lineages
    pq = ws.gcmh_problem(genes, codes, strata, 2)
    qrows = [gs.perm_row(SEED, 0, pi, codes, strata, 2) for pi in range(P)]
    cells = ws.gcmh_cells(genes, qrows, pq, strata, 2)
    rq = ws.r_fwer(ws.maxs(cells), pq["thr"])
    r_own = (cells >= np.array(pq["thr"])[None, :]).sum(axis=0)
    head, lines = _split(data["fwer_s"]["host.gcmh.results.csv"])
    assert head[-2:] == ["Empirical_p", "Westfall_Young_p"] and len(lines) == 7
    for line in lines:
        g = int(line[0][1:])
        assert line[-2:] == [m._fmt((int(r_own[g]) + 1.0) / (P + 1.0)), m._fmt((int(rq[g]) + 1.0) / (P + 1.0))], g
    # within the lineages the marker is unremarkable and the gene that follows the label leads the family
    assert rq[1] == 0 and rq[0] > P // 4


def test_the_refusals_exit_with_their_messages(data, monkeypatch):
    from scoary_amd import methods as m
    base = [a for a in data["common"] if a not in ("-e", str(P))]
    for argv, text in ((base + [FLAG], m.CAT_WY_TEXT["permute"]),
                       (base[:base.index("--categorical")] + ["-e", str(P), FLAG], m.CAT_WY_TEXT["categorical"])):
        monkeypatch.setattr(sys, "argv", ["scoary"] + argv + ["-o", str(data["dir"] / "out_refused"), "--no-time"])
        with pytest.raises(SystemExit) as e:
            m.main()
        assert e.value.code == text
