"""--categorical-strata FILE through main(): a 40-isolate table with a 3-class and a 2-class trait over three lineages,
run with the flag (with --permute 60 and without permutations) and without it -- the new files, their columns, their
row order and every cell against the engine's calls and the restatement (gcmh_spec.py), and every other result file
byte for byte the same in both runs; and the clonal population the test exists for, where the chi-square test of a
lineage marker is tiny and the stratified one is not."""
import csv
import io
import os

import numpy as np
import pytest

import categorical_spec as cs
import gcmh_spec as gs
from cmh_homog_spec import chi2_sf
from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
G, N, P, SEED, S = 75, 40, 60, 777, 3
COLUMNS = ["Gene", "Non-unique Gene name", "Annotation", "Number_with_gene", "Number_without_gene", "Carriers_by_class",
           "Expected_by_class", "Most_enriched_class", "GCMH", "GCMH_df", "GCMH_p", "Bonferroni_p", "Benjamini_H_p"]
META = ["Gene", "Non-unique Gene name", "Annotation", "No. isolates", "No. sequences", "Avg sequences per isolate",
        "Genome Fragment", "Order within Fragment", "Accessory Fragment", "Accessory Order with Fragment", "QC",
        "Min group size nuc", "Max group size nuc", "Avg group size nuc"]


def _write_table(path, dense, iso):
    cells = np.where(np.asarray(dense, dtype=bool), "x", "")
    path.write_text(",".join(META + iso) + "\n" + "".join(
        "g%03d,nu%d,\"an, %d\",%s,%s\n" % (g, g, g, ",".join(["1"] * 11), ",".join(cells[g])) for g in range(len(cells))))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    rng = np.random.default_rng(45)
    d = tmp_path_factory.mktemp("gcmh_cli")
    dense = rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))
    dense[5], dense[6] = False, True
    host = [["pig", "cattle", "human"][k] for k in rng.integers(0, 3, N)]     # sorted: cattle, human, pig
    source = [["blood", "Faeces"][k] for k in rng.integers(0, 2, N)]          # sorted as strings: Faeces, blood
    lineage = ["L%d" % k for k in rng.integers(0, S, N)]
    for i in (3, 14, 25):
        host[i] = None
    source[8] = None
    iso = ["s%02d" % i for i in range(N)]
    _write_table(d / "g.csv", dense, iso)
    (d / "t.csv").write_text(",bin\n" + "".join("%s,%d\n" % (iso[i], i % 3 == 0) for i in range(N)))
    (d / "c.csv").write_text("Name,host,source\n" + "".join(
        "%s,%s,%s\n" % (iso[i], host[i] or "NA", source[i] or "-") for i in range(N)) + "other,llama,soil\n")
    (d / "s.csv").write_text("Isolate,Lineage\n" + "".join("%s,%s\n" % (iso[i], lineage[i]) for i in range(N))
                             + "other,L9\n")
    common = ["-g", str(d / "g.csv"), "-t", str(d / "t.csv"), "--no_pairwise", "--seed", str(SEED), "-p", "1.0",
              "--categorical", str(d / "c.csv")]
    flag = ["--categorical-strata", str(d / "s.csv")]
    labels = sorted(set(lineage), key=lineage.index)                         # numbered in order of first appearance
    return dict(dense=dense.astype(np.uint8), labels=[host, source], strata=[labels.index(x) for x in lineage], dir=d,
                with_s=run_cli(common + ["-e", str(P)] + flag, d / "out_s"),
                without=run_cli(common + ["-e", str(P)], d / "out_plain"),
                no_perm=run_cli(common + flag + ["-m", "7"], d / "out_noperm"))


def test_every_other_result_file_is_byte_identical(data):
    assert sorted(data["without"]) == ["bin.results.csv", "host.categorical.results.csv",
                                       "source.categorical.results.csv"]
    assert sorted(data["with_s"]) == sorted(list(data["without"]) + ["host.gcmh.results.csv", "source.gcmh.results.csv"])
    for name, text in data["without"].items():
        assert data["with_s"][name] == text and len(text.splitlines()) > 10


def test_gcmh_files_hold_what_the_engine_returns_and_the_restatement(data):
    from scoary_amd import _abi, methods as m
    assert _abi.ABI_VERSION == 11
    eng = m.get_engine()
    gm = eng.pack_dense(data["dense"])
    spec = [cs.codes_of(row) for row in data["labels"]]
    codes = np.array([s[1] for s in spec])
    strata = np.array(data["strata"])
    assert sorted(set(data["strata"])) == list(range(S))
    plan = eng.gcmh_plan(codes, strata)
    res = eng.gcmh(gm, plan)
    r = eng.gcmh_permute(gm, plan, res, P, SEED).cpu().numpy()
    a, e, mm, q, df, p = (res[k].cpu().numpy() for k in ("a", "e", "m", "q", "df", "p"))
    for t, name in enumerate(("host", "source")):
        classes, row = spec[t]
        K = len(classes)
        nsk = gs.margins(row, data["strata"], S)
        n = sum(map(sum, nsk))
        rows_spec = [gs.perm_row(SEED, t, pi, row, data["strata"], S) for pi in range(P)]
        text = data["with_s"][name + ".gcmh.results.csv"]
        assert all(line.startswith('"') and line.endswith('"') for line in text.splitlines())
        rows = list(csv.reader(io.StringIO(text)))
        assert rows[0] == COLUMNS + ["Empirical_p"]
        stats = {}
        for g in range(G):
            tab, ms = gs.counts(data["dense"][g].tolist(), row, data["strata"], S)
            stats[g] = (tab, ms, gs.statistic(tab, ms, nsk))
        testable = [g for g in range(G) if stats[g][2]["df"] > 0]
        assert 5 not in testable and 6 not in testable and len(rows) - 1 == len(testable) >= G - 8
        order = sorted(testable, key=lambda g: (p[t, g], g))             # ascending p, ties in file order
        assert [line[0] for line in rows[1:]] == ["g%03d" % g for g in order]
        bonf, bh = m.bonferroni_bh(p[t, testable], len(testable))
        for line in rows[1:]:
            g = int(line[0][1:])
            k = testable.index(g)
            tab, ms, st = stats[g]
            assert a[t, g].tolist() == tab and e[t, g].tolist() == st["E"] and q[t, g] == st["q"] and df[t, g] == st["df"]
            sp = chi2_sf(st["q"], st["df"])
            assert abs(p[t, g] - sp) <= 1e-10 * sp
            r_spec = sum(1 for prow in rows_spec
                         if gs.q_of(gs.counts(data["dense"][g].tolist(), prow, data["strata"], S)[0], st["form"]) >= st["thr"])
            assert int(r[t, g]) == r_spec
            assert line[1:3] == ["nu%d" % g, "an, %d" % g]
            assert line[3:] == [m._fmt(sum(tab)), m._fmt(n - sum(tab)),
                                "|".join("%s=%d" % (c, x) for c, x in zip(classes, tab)),
                                "|".join("%s=%s" % (c, repr(x)) for c, x in zip(classes, st["E"])),
                                classes[gs.most_enriched(tab[:K], st["E"][:K])], repr(st["q"]), str(st["df"]),
                                m._fmt(p[t, g]), m._fmt(bonf[k]), m._fmt(bh[k]),
                                m._fmt((int(r[t, g]) + 1.0) / (P + 1.0))]


def test_max_hits_and_no_permutations(data):
    whole = list(csv.reader(io.StringIO(data["with_s"]["host.gcmh.results.csv"])))
    got = list(csv.reader(io.StringIO(data["no_perm"]["host.gcmh.results.csv"])))
    assert got[0] == COLUMNS and len(got) == 8                               # no Empirical_p, seven rows
    assert got[1:] == [row[:-1] for row in whole[1:8]]
    log = open(os.path.join(str(data["dir"] / "out_noperm"), "scoary.log")).read()
    assert "Generalized CMH test of host: %d isolates with a label in 3 classes and 3 strata" % (N - 3) in log


def test_a_lineage_marker_is_tiny_pooled_and_unremarkable_within_the_lineages(tmp_path):
    """Two lineages, the label follows the lineage: the marker gene has Chi2_p < 1e-6 and GCMH_p > 0.05, the gene that
    follows the label inside the lineages keeps GCMH_p < 1e-3."""
    genes, labels, strata = gs.clonal_scenario()
    iso = ["i%03d" % i for i in range(len(labels))]
    _write_table(tmp_path / "g.csv", genes, iso)
    (tmp_path / "t.csv").write_text(",bin\n" + "".join("%s,%d\n" % (s, i % 2) for i, s in enumerate(iso)))
    (tmp_path / "c.csv").write_text("Name,host\n" + "".join("%s,%s\n" % x for x in zip(iso, labels)))
    (tmp_path / "s.csv").write_text("Isolate,Lineage\n" + "".join("%s,L%d\n" % x for x in zip(iso, strata)))
    out = run_cli(["-g", str(tmp_path / "g.csv"), "-t", str(tmp_path / "t.csv"), "--no_pairwise", "-p", "1.0",
                   "--categorical", str(tmp_path / "c.csv"), "--categorical-strata", str(tmp_path / "s.csv")],
                  tmp_path / "out")
    chi = {row["Gene"]: float(row["Chi2_p"]) for row in csv.DictReader(io.StringIO(out["host.categorical.results.csv"]))}
    gcmh = {row["Gene"]: float(row["GCMH_p"]) for row in csv.DictReader(io.StringIO(out["host.gcmh.results.csv"]))}
    assert chi["g000"] < 1e-6 and gcmh["g000"] > 0.05
    assert gcmh["g001"] < 1e-3
    assert gcmh["g002"] > 0.05 and chi["g002"] > 0.05
