"""--covariates-spa through main(): one synthetic table of 80 genes x 60 isolates with a balanced and a rare binary
trait, a measured trait and two covariates, run with --covariates alone, with --covariates-spa and with a cutoff of
its own -- the logistic files with the flag, less their four last columns, are the files without it byte for byte,
every new cell is engine.score_spa's and bonferroni_bh's, the linear files and every other file are the same bytes,
and the log names the genes that went to the saddlepoint."""
import csv
import io
import os

import numpy as np
import pytest

from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
G, N = 80, 60
SPA = ["SPA_p", "SPA_Bonferroni_p", "SPA_Benjamini_H_p", "SPA_status"]


def _cell(x):
    return "NA" if np.isnan(x) else repr(float(x))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    rng = np.random.default_rng(2525)
    d = tmp_path_factory.mktemp("score_spa_cli")
    cov = rng.standard_normal((2, N))
    dense = rng.random((G, N)) < rng.uniform(0.05, 0.6, (G, 1))
    dense[7] = rng.random(N) < 0.4
    binary = np.stack([rng.random(N) < 1 / (1 + np.exp(-(cov[0] + 2.5 * dense[7] - 1.0))),
                       rng.random(N) < 0.15]).astype(np.float64)
    dense[8] = (binary[1] == 1) & (rng.random(N) < 0.8)                        # a rare gene of the rare trait
    measured = (cov[0] + rng.standard_normal(N))[None, :]
    binary[0, 3::17] = np.nan
    cov[1, 11] = np.nan
    iso = ["s%03d" % i for i in range(N)]
    meta = ["Gene", "Non-unique Gene name", "Annotation", "No. isolates", "No. sequences",
            "Avg sequences per isolate", "Genome Fragment", "Order within Fragment", "Accessory Fragment",
            "Accessory Order with Fragment", "QC", "Min group size nuc", "Max group size nuc", "Avg group size nuc"]
    cells = np.where(dense, "x", "")
    (d / "g.csv").write_text(",".join(meta + iso) + "\n" + "".join(
        "g%03d,nu%d,an%d,%s,%s\n" % (g, g, g, ",".join(["1"] * 11), ",".join(cells[g])) for g in range(G)))
    (d / "t.csv").write_text(",res,rare\n" + "".join(
        "%s,%s,%s\n" % (iso[i], *("NA" if np.isnan(v) else str(int(v)) for v in binary[:, i])) for i in range(N)))
    (d / "q.csv").write_text("Name,mic\n" + "".join("%s,%s\n" % (iso[i], _cell(measured[0, i])) for i in range(N)))
    (d / "c.csv").write_text("Name,pc1,pc2\n" + "".join(
        "%s,%s\n" % (iso[i], ",".join(_cell(x) for x in cov[:, i])) for i in range(N)))
    common = ["-g", str(d / "g.csv"), "-t", str(d / "t.csv"), "--no_pairwise", "-p", "1.0", "--quantitative",
              str(d / "q.csv"), "--covariates", str(d / "c.csv")]
    runs = {"plain": run_cli(common, d / "out_plain"),
            "spa": run_cli(common + ["--covariates-spa"], d / "out_spa"),
            "low": run_cli(common + ["--covariates-spa", "--covariates-spa-cutoff", "0.5", "-m", "9"], d / "out_low")}
    return dict(dense=dense.astype(np.uint8), binary=binary, cov=cov, runs=runs, dir=d)


def test_only_the_four_last_columns_are_new(data):
    plain, spa, low = (data["runs"][k] for k in ("plain", "spa", "low"))
    assert sorted(plain) == sorted(spa) == sorted(low)
    assert sorted(plain) == ["mic.linear.results.csv", "mic.ranksum.results.csv", "rare.logistic.results.csv",
                             "rare.results.csv", "res.logistic.results.csv", "res.results.csv"]
    for name, text in plain.items():
        if not name.endswith(".logistic.results.csv"):
            assert spa[name] == text, name                                     # the linear file among them
            continue
        rows, rows_spa = text.splitlines(), spa[name].splitlines()
        assert len(rows) == len(rows_spa) > 20
        for a, b in zip(rows, rows_spa):
            cells = b.split(",")
            assert ",".join(cells[:-4]) == a and len(cells) == len(a.split(",")) + 4
        assert [c.strip('"') for c in rows_spa[0].split(",")[-4:]] == SPA
        cut = low[name].splitlines()                                           # -m 9 cuts by Score_p, as it does without
        assert len(cut) == 10 and [",".join(r.split(",")[:-4]) for r in cut] == rows[:10]


@pytest.mark.parametrize("run,cutoff", [("spa", 2.0), ("low", 0.5)])
def test_the_new_cells_are_the_engines(data, run, cutoff):
    from scoary_amd import methods as m
    eng = m.get_engine()
    gm = eng.pack_dense(data["dense"])
    plan = eng.score_plan(data["binary"], data["cov"], "logistic")
    assert plan.skipped == [None, None]
    score = eng.score(gm, plan)
    spa = {k: v.cpu().numpy() for k, v in eng.score_spa(gm, plan, score, cutoff).items()}
    res = {k: v.cpu().numpy() for k, v in score.items()}
    seen = set()
    for t, name in enumerate(("res", "rare")):
        rows = list(csv.reader(io.StringIO(data["runs"][run]["%s.logistic.results.csv" % name])))
        n = int(plan.n[t])
        testable = [g for g in range(G) if 0 < res["m"][t, g] < n and res["Vg"][t, g] > 2.0 ** -26 * res["b"][t, g, 0]]
        bonf, bh = m.bonferroni_bh(spa["p"][t][testable], len(testable))
        assert len(rows) - 1 == (len(testable) if run == "spa" else 9)
        for row in rows[1:]:
            g = int(row[0][1:])
            k = testable.index(g)
            assert row[-4:] == [m._fmt(spa["p"][t, g]), m._fmt(bonf[k]), m._fmt(bh[k]), m._fmt(int(spa["status"][t, g]))]
            assert (spa["status"][t, g] == 0) == (res["stat"][t, g] < cutoff * cutoff)
            if spa["status"][t, g] != 1:
                assert row[-4] == row[9]                                        # SPA_p is Score_p's cell
            seen.add(int(spa["status"][t, g]))
    assert seen == ({0, 1} if run == "spa" else {1})                          # -m 9 shows the strongest rows only
    log = open(os.path.join(str(data["dir"] / ("out_" + run)), "scoary.log")).read()
    for t, name in enumerate(("res", "rare")):
        n = int(plan.n[t])
        ok = (res["m"][t] > 0) & (res["m"][t] < n) & (res["Vg"][t] > 2.0 ** -26 * res["b"][t, :, 0])
        status = spa["status"][t][ok]
        line = ("Saddlepoint p of %s: %d of its %d tested genes are at or above the cutoff of %s standard deviations, "
                "%d of them fell back to Score_p" % (name, int((status != 0).sum()), len(status), m._fmt(cutoff),
                                                      int((status == 2).sum())))
        assert line in log, line
    assert "Saddlepoint" not in open(os.path.join(str(data["dir"] / "out_plain"), "scoary.log")).read()
