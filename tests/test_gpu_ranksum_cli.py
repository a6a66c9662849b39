"""--quantitative FILE through main(): one small synthetic data set, run with the flag (and --permute 50) and without
it -- the new files, their columns, their row order and every cell against the engine's calls, and every ordinary
result file byte for byte the same in both runs."""
import csv
import io
import os

import numpy as np
import pytest

from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
G, N, P, SEED = 90, 61, 50, 4242
COLUMNS = ["Gene", "Non-unique Gene name", "Annotation", "Number_with_gene", "Number_without_gene", "Rank_sum_AUC",
           "Rank_sum_p", "Bonferroni_p", "Benjamini_H_p"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    rng = np.random.default_rng(33)
    d = tmp_path_factory.mktemp("ranksum_cli")
    dense = rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))
    dense[5], dense[6] = False, True
    mic = np.round(np.exp2(rng.integers(-3, 4, N).astype(float)), 3)          # MIC-like: heavy ties
    dense[7] = rng.random(N) < 0.5
    mic[dense[7]] += 100.0                                                    # gene 7 carries the phenotype: AUC 1
    growth = rng.standard_normal(N)
    iso = ["s%02d" % i for i in range(N)]
    meta = ["Gene", "Non-unique Gene name", "Annotation", "No. isolates", "No. sequences",
            "Avg sequences per isolate", "Genome Fragment", "Order within Fragment",
            "Accessory Fragment", "Accessory Order with Fragment", "QC", "Min group size nuc",
            "Max group size nuc", "Avg group size nuc"]
    cells = np.where(dense, "x", "")
    (d / "g.csv").write_text(",".join(meta + iso) + "\n" + "".join(
        "g%03d,nu%d,\"an, %d\",%s,%s\n" % (g, g, g, ",".join(["1"] * 11), ",".join(cells[g])) for g in range(G)))
    (d / "t.csv").write_text(",bin\n" + "".join("%s,%d\n" % (iso[i], mic[i] % 100 > 1) for i in range(N)))
    qrows = []
    for i in range(N):
        if i == 9:
            continue                                                          # absent from the file: missing
        qrows.append("%s,%s,%s\n" % (iso[i], "NA" if i % 11 == 3 else repr(float(mic[i])), repr(float(growth[i]))))
    (d / "q.csv").write_text("Name,mic,growth\n" + "".join(qrows) + "other,1,2\n")
    vals = np.stack([mic, growth])
    vals[:, 9] = np.nan
    vals[0, 3::11] = np.nan
    common = ["-g", str(d / "g.csv"), "-t", str(d / "t.csv"), "--no_pairwise", "-e", str(P), "--seed", str(SEED),
              "-p", "1.0"]
    with_q = run_cli(common + ["--quantitative", str(d / "q.csv")], d / "out_q")
    without = run_cli(common, d / "out_plain")
    return dict(dense=dense.astype(np.uint8), vals=vals, with_q=with_q, without=without, dir=d, common=common)


def test_ordinary_result_files_are_byte_identical(data):
    assert sorted(data["without"]) == ["bin.results.csv"]
    assert sorted(data["with_q"]) == ["bin.results.csv", "growth.ranksum.results.csv", "mic.ranksum.results.csv"]
    assert data["with_q"]["bin.results.csv"] == data["without"]["bin.results.csv"]
    assert len(data["without"]["bin.results.csv"].splitlines()) > 10


def test_rank_sum_files_hold_what_the_engine_returns(data):
    from scoary_amd import methods as m
    eng = m.get_engine()
    gm = eng.pack_dense(data["dense"])
    plan = eng.ranksum_plan(data["vals"])
    res = eng.ranksum(gm, plan)
    r = eng.ranksum_permute(gm, plan, res["d"], P, SEED).cpu().numpy()
    mm, auc, p = (res[k].cpu().numpy() for k in ("m", "auc", "p"))
    for t, name in enumerate(("mic", "growth")):
        text = data["with_q"][name + ".ranksum.results.csv"]
        assert all(line.startswith('"') and line.endswith('"') for line in text.splitlines())
        rows = list(csv.reader(io.StringIO(text)))
        assert rows[0] == COLUMNS + ["Empirical_p"]
        n = int(plan.n[t])
        testable = [g for g in range(G) if 0 < mm[t, g] < n]
        assert 5 not in testable and 6 not in testable and len(rows) - 1 == len(testable) >= G - 4
        order = sorted(testable, key=lambda g: (p[t, g], g))             # ascending p, ties in file order
        assert [row[0] for row in rows[1:]] == ["g%03d" % g for g in order]
        bonf, bh = m.bonferroni_bh(p[t, testable], len(testable))
        for row in rows[1:]:
            g = int(row[0][1:])
            k = testable.index(g)
            assert row[1:3] == ["nu%d" % g, "an, %d" % g]
            assert row[3:] == [m._fmt(int(mm[t, g])), m._fmt(n - int(mm[t, g])), m._fmt(auc[t, g]), m._fmt(p[t, g]),
                               m._fmt(bonf[k]), m._fmt(bh[k]), m._fmt((int(r[t, g]) + 1.0) / (P + 1.0))]
    top = list(csv.reader(io.StringIO(data["with_q"]["mic.ranksum.results.csv"])))[1]
    assert top[0] == "g007" and top[5] == "1.0"                               # the planted gene is the top hit
    assert plan.n.tolist() == [N - 1 - len(range(3, N, 11)), N - 1]           # isolate 9 absent, six NA cells


def test_max_hits_semicolon_and_no_permutations(data):
    d = data["dir"]
    q = d / "q_semi.csv"
    q.write_text((d / "q.csv").read_text().replace(",", ";"))
    g = d / "g_semi.csv"
    # (the gene table's annotation holds a quoted comma: rewritten cell by cell)
    rows = list(csv.reader(io.StringIO((d / "g.csv").read_text())))
    g.write_text("".join(";".join(r) + "\n" for r in rows))
    t = d / "t_semi.csv"
    t.write_text((d / "t.csv").read_text().replace(",", ";"))
    files = run_cli(["-g", str(g), "-t", str(t), "--no_pairwise", "--delimiter", ";", "-m", "7", "-p", "1.0",
                     "--quantitative", str(q)], d / "out_semi")
    whole = list(csv.reader(io.StringIO(data["with_q"]["mic.ranksum.results.csv"])))
    got = list(csv.reader(io.StringIO(files["mic.ranksum.results.csv"]), delimiter=";"))
    assert got[0] == COLUMNS and len(got) == 8                               # no Empirical_p, seven rows
    assert got[1:] == [row[:-1] for row in whole[1:8]]
    log = open(os.path.join(str(d / "out_semi"), "scoary.log")).read()
    assert "Rank-sum test of mic: %d isolates with a value" % (N - 1 - 6) in log and "tie groups" in log
