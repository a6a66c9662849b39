"""--covariates FILE through main(): one synthetic table of 300 genes x 120 isolates with two binary traits, two
measured traits, three covariates and some missing cells, run with the flag and without it -- the four new files,
their columns, their row order and every cell against the engine's calls and the host corrections, every other
result file byte for byte the same in both runs; and a trait that a covariate separates, skipped with its warning."""
import csv
import io
import os

import numpy as np
import pytest

from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
G, N, P, SEED = 300, 120, 20, 777
HEAD = ["Gene", "Non-unique Gene name", "Annotation"]
LOGISTIC = HEAD + ["Number_with_gene", "Number_without_gene", "Beta", "Std_err", "Odds_ratio", "Score_chi2", "Score_p",
                   "Bonferroni_p", "Benjamini_H_p"]
LINEAR = HEAD + ["Number_with_gene", "Number_without_gene", "Beta", "Std_err", "T_stat", "Linear_p", "Bonferroni_p",
                 "Benjamini_H_p"]


def _cell(x):
    return "NA" if np.isnan(x) else repr(float(x))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    rng = np.random.default_rng(2424)
    d = tmp_path_factory.mktemp("score_cli")
    cov = rng.standard_normal((3, N))
    cov[2] = 2000 + rng.integers(0, 20, N)                                     # a sampling year
    dense = rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))
    dense[5], dense[6] = False, True
    dense[7] = rng.random(N) < 0.5
    binary = np.stack([rng.random(N) < 1 / (1 + np.exp(-(cov[0] + 2.5 * dense[7] - 1.2))),
                       rng.random(N) < 1 / (1 + np.exp(-cov[1]))]).astype(np.float64)
    measured = np.stack([cov[0] + 1.5 * dense[7] + rng.standard_normal(N), rng.standard_normal(N)])
    binary[0, 3::17] = np.nan
    measured[0, 5::13] = np.nan
    cov[1, 11] = cov[0, 40] = np.nan
    iso = ["s%03d" % i for i in range(N)]
    meta = HEAD + ["No. isolates", "No. sequences", "Avg sequences per isolate", "Genome Fragment",
                   "Order within Fragment", "Accessory Fragment", "Accessory Order with Fragment", "QC",
                   "Min group size nuc", "Max group size nuc", "Avg group size nuc"]
    cells = np.where(dense, "x", "")
    (d / "g.csv").write_text(",".join(meta + iso) + "\n" + "".join(
        "g%03d,nu%d,\"an, %d\",%s,%s\n" % (g, g, g, ",".join(["1"] * 11), ",".join(cells[g])) for g in range(G)))
    (d / "t.csv").write_text(",res,vir\n" + "".join(
        "%s,%s,%s\n" % (iso[i], *("NA" if np.isnan(v) else str(int(v)) for v in binary[:, i])) for i in range(N)))
    (d / "q.csv").write_text("Name,mic,growth\n" + "".join(
        "%s,%s,%s\n" % (iso[i], _cell(measured[0, i]), _cell(measured[1, i])) for i in range(N)))
    crows = ["%s,%s\n" % (iso[i], ",".join(_cell(x) for x in cov[:, i])) for i in range(N) if i != 9]
    (d / "c.csv").write_text("Name,pc1,pc2,year\n" + "".join(crows) + "other,1,2,3\n")
    cov[:, 9] = np.nan                                                         # absent from the file: missing
    common = ["-g", str(d / "g.csv"), "-t", str(d / "t.csv"), "--no_pairwise", "-e", str(P), "--seed", str(SEED),
              "-p", "1.0", "--quantitative", str(d / "q.csv")]
    with_c = run_cli(common + ["--covariates", str(d / "c.csv")], d / "out_c")
    without = run_cli(common, d / "out_plain")
    return dict(dense=dense.astype(np.uint8), binary=binary, measured=measured, cov=cov, with_c=with_c,
                without=without, dir=d, common=common, iso=iso)


def test_every_other_result_file_is_byte_identical(data):
    new = ["growth.linear.results.csv", "mic.linear.results.csv", "res.logistic.results.csv",
           "vir.logistic.results.csv"]
    assert sorted(data["without"]) == ["growth.ranksum.results.csv", "mic.ranksum.results.csv", "res.results.csv",
                                       "vir.results.csv"]
    assert sorted(data["with_c"]) == sorted(new + list(data["without"]))
    for name, text in data["without"].items():
        assert data["with_c"][name] == text, name
        assert len(text.splitlines()) > 10


@pytest.mark.parametrize("kind", ["logistic", "linear"])
def test_score_files_hold_what_the_engine_returns(data, kind):
    from scoary_amd import methods as m
    eng = m.get_engine()
    gm = eng.pack_dense(data["dense"])
    values, names = (data["binary"], ("res", "vir")) if kind == "logistic" else (data["measured"], ("mic", "growth"))
    plan = eng.score_plan(values, data["cov"], kind)
    assert plan.skipped == [None, None] and plan.q == 4
    res = {k: v.cpu().numpy() for k, v in eng.score(gm, plan).items()}
    stat = res["t" if kind == "linear" else "stat"]
    for t, name in enumerate(names):
        text = data["with_c"]["%s.%s.results.csv" % (name, kind)]
        assert all(line.startswith('"') and line.endswith('"') for line in text.splitlines())
        rows = list(csv.reader(io.StringIO(text)))
        assert rows[0] == (LOGISTIC if kind == "logistic" else LINEAR)       # --permute adds nothing
        n = int(plan.n[t])
        mm, p = res["m"][t], res["p"][t]
        testable = [g for g in range(G) if 0 < mm[g] < n and res["Vg"][t, g] > 2.0 ** -26 * res["b"][t, g, 0]]
        assert 5 not in testable and 6 not in testable and len(rows) - 1 == len(testable) >= G - 10
        order = sorted(testable, key=lambda g: (p[g], g))                     # ascending p, ties in file order
        assert [row[0] for row in rows[1:]] == ["g%03d" % g for g in order]
        bonf, bh = m.bonferroni_bh(p[testable], len(testable))
        for row in rows[1:]:
            g = int(row[0][1:])
            k = testable.index(g)
            beta = float(res["beta"][t, g])
            own = [m._fmt(beta), m._fmt(res["se"][t, g])]
            own += [m._fmt(float(np.exp(beta))), m._fmt(stat[t, g])] if kind == "logistic" else [m._fmt(stat[t, g])]
            assert row[1:3] == ["nu%d" % g, "an, %d" % g]
            assert row[3:] == [m._fmt(int(mm[g])), m._fmt(n - int(mm[g]))] + own + \
                [m._fmt(p[g]), m._fmt(bonf[k]), m._fmt(bh[k])]
    top = list(csv.reader(io.StringIO(data["with_c"]["%s.%s.results.csv" % (names[0], kind)])))[1]
    assert top[0] == "g007" and float(top[5]) > 0                              # the planted gene is the top hit
    valid = ~np.isnan(data["cov"]).any(axis=0)
    assert plan.n.tolist() == [int((valid & ~np.isnan(v)).sum()) for v in values]
    assert valid.sum() == N - 3


def test_a_separated_trait_is_skipped_with_its_warning(data):
    """A binary trait that a covariate separates: one warning line, no file for it, the other trait's file as it
    was, and the run exits 0."""
    d = data["dir"]
    cov0 = np.nan_to_num(data["cov"][0])
    (d / "t_sep.csv").write_text(",res,split\n" + "".join(
        "%s,%s,%d\n" % (data["iso"][i], "NA" if np.isnan(data["binary"][0, i]) else str(int(data["binary"][0, i])),
                        cov0[i] > 0.2) for i in range(N)))
    files = run_cli(["-g", str(d / "g.csv"), "-t", str(d / "t_sep.csv"), "--no_pairwise", "-p", "1.0", "-m", "7",
                     "--covariates", str(d / "c.csv")], d / "out_sep")
    assert sorted(files) == ["res.logistic.results.csv", "res.results.csv", "split.results.csv"]
    whole = data["with_c"]["res.logistic.results.csv"].splitlines()
    assert files["res.logistic.results.csv"].splitlines() == whole[:8]         # -m 7: the header and seven rows
    log = open(os.path.join(str(d / "out_sep"), "scoary.log")).read()
    lines = [line for line in log.splitlines() if "Skipping the logistic score test of split" in line]
    assert len(lines) == 1 and "the covariates separate its classes" in lines[0]
    assert "No results file is written for it" in lines[0]
    assert "Logistic score test of res next to 3 covariates" in log
