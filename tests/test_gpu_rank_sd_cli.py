"""--quantitative-fwer-stepdown through main(): test_gpu_rank_wy_cli's small synthetic data set (60 genes x 40
isolates, two measured traits, four strata), --permute 50, run with the flag and without it, with
--quantitative-fwer and without it, with --quantitative-strata and without it.  The new column is (r_sd + 1) /
(P + 1) of the restatement (rank_sd_spec.py) from the seed alone and of the engine, it lies between Empirical_p and
Westfall_Young_p, every other cell is the cell of the run without the flag, and without the flag two runs write the
same bytes."""
import csv
import io

import numpy as np
import pytest

import rank_sd_spec as sd
import rank_wy_spec as wy
import ranksum_spec as rsp
import vanelteren_spec as vsp
from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
G, N, P, SEED, S = 60, 40, 50, 4242, 4
RANK_FILES = ["growth.ranksum.results.csv", "mic.ranksum.results.csv"]
STRATA_FILES = ["growth.vanelteren.results.csv", "mic.vanelteren.results.csv"]
COLUMN = "Westfall_Young_stepdown_p"


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    rng = np.random.default_rng(60)
    d = tmp_path_factory.mktemp("rank_sd_cli")
    dense = rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))
    dense[5], dense[6] = False, True
    mic = np.round(np.exp2(rng.integers(-3, 4, N).astype(float)), 3)          # MIC-like: heavy ties
    dense[7] = rng.random(N) < 0.5
    mic[dense[7]] += 100.0                                                    # gene 7 carries the phenotype
    dense[8] = dense[7]                                                       # ... and gene 8 is its copy: a tie group
    growth = rng.standard_normal(N)
    iso = ["s%02d" % i for i in range(N)]
    meta = ["Gene", "Non-unique Gene name", "Annotation", "No. isolates", "No. sequences",
            "Avg sequences per isolate", "Genome Fragment", "Order within Fragment",
            "Accessory Fragment", "Accessory Order with Fragment", "QC", "Min group size nuc",
            "Max group size nuc", "Avg group size nuc"]
    cells = np.where(dense, "x", "")
    (d / "g.csv").write_text(",".join(meta + iso) + "\n" + "".join(
        "g%03d,nu%d,an%d,%s,%s\n" % (g, g, g, ",".join(["1"] * 11), ",".join(cells[g])) for g in range(G)))
    (d / "t.csv").write_text(",bin\n" + "".join("%s,%d\n" % (iso[i], mic[i] % 100 > 1) for i in range(N)))
    vals = np.stack([mic, growth])
    vals[0, 3::11] = np.nan
    vals[1, 9] = np.nan
    (d / "q.csv").write_text("Name,mic,growth\n" + "".join(
        "%s,%s,%s\n" % (iso[i], *("NA" if np.isnan(v) else repr(float(v)) for v in vals[:, i])) for i in range(N)))
    labels = ["solo" if i == 0 else "pair" if i in (1, 2) else "clade %d" % (i % 2) for i in range(N)]
    (d / "strata.csv").write_text("Isolate,Lineage\n" + "".join("%s,%s\n" % kv for kv in zip(iso, labels)))
    index = {}
    st = [index.setdefault(lab, len(index)) for lab in labels]               # by first appearance: sizes 1, 2, 19, 18
    common = ["-g", str(d / "g.csv"), "-t", str(d / "t.csv"), "--no_pairwise", "-e", str(P), "--seed", str(SEED),
              "-p", "1.0", "--quantitative", str(d / "q.csv")]
    strata = ["--quantitative-strata", str(d / "strata.csv")]
    flag = ["--quantitative-fwer-stepdown"]
    runs = dict(both_strata=run_cli(common + strata + ["--quantitative-fwer"] + flag, d / "out_bs"),
                sd_strata=run_cli(common + strata + flag, d / "out_ds"),
                sd=run_cli(common + flag, d / "out_d"),
                fwer_strata=run_cli(common + strata + ["--quantitative-fwer"], d / "out_fs"),
                plain_strata=run_cli(common + strata, d / "out_s"),
                plain_strata_again=run_cli(common + strata, d / "out_s2"))
    return dict(dense=dense.astype(np.int64), vals=vals, st=st, runs=runs)


def _rows(text):
    assert all(line.startswith('"') and line.endswith('"') for line in text.splitlines())
    return list(csv.reader(io.StringIO(text)))


def test_without_the_flag_the_files_do_not_change(data):
    runs = data["runs"]
    assert sorted(runs["plain_strata"]) == sorted(["bin.results.csv"] + RANK_FILES + STRATA_FILES)
    assert runs["plain_strata"] == runs["plain_strata_again"]                 # byte for byte
    for name in RANK_FILES + STRATA_FILES:
        assert _rows(runs["plain_strata"][name])[0][-1] == "Empirical_p"
        head = _rows(runs["fwer_strata"][name])[0]
        assert head[-2:] == ["Empirical_p", "Westfall_Young_p"] and COLUMN not in head
    assert sorted(runs["both_strata"]) == sorted(runs["sd_strata"]) == sorted(runs["plain_strata"])
    assert sorted(runs["sd"]) == sorted(["bin.results.csv"] + RANK_FILES)
    for run in ("both_strata", "sd_strata", "sd", "fwer_strata"):
        assert runs[run]["bin.results.csv"] == runs["plain_strata"]["bin.results.csv"]
    assert len(runs["plain_strata"]["bin.results.csv"].splitlines()) > 10


def test_every_other_cell_is_the_run_without_the_flag(data):
    """Two runs in one test, column by column: with the flag and without it, under --quantitative-fwer and not."""
    runs = data["runs"]
    for name in RANK_FILES + STRATA_FILES:
        for with_flag, without, before in (("sd_strata", "plain_strata", "Empirical_p"),
                                           ("both_strata", "fwer_strata", "Westfall_Young_p")):
            got, want = _rows(runs[with_flag][name]), _rows(runs[without][name])
            assert got[0] == want[0] + [COLUMN] and want[0][-1] == before and len(got) == len(want) > 20
            assert [row[:-1] for row in got] == want, (name, with_flag)
        for row in _rows(runs["both_strata"][name])[1:]:                      # Empirical <= step-down <= single-step
            assert float(row[-3]) <= float(row[-1]) <= float(row[-2]) <= 1 and float(row[-1]) > 0, (name, row[0])
        # the column does not depend on the other flag
        assert [row[-1] for row in _rows(runs["both_strata"][name])] == [row[-1] for row in _rows(runs["sd_strata"][name])]
    for name in RANK_FILES:                                          # the strata change nothing in the rank-sum files
        assert runs["sd"][name] == runs["sd_strata"][name]


def _expected(data, t, strata):
    """(problem, r, r_fwer, r_sd) of trait t from the restatements and the seed."""
    genes = data["dense"].tolist()
    vals = [float(v) for v in data["vals"][t]]
    if strata:
        pr = wy.vanelteren_problem(genes, vals, data["st"], S)
        rows = [vsp.perm_row(SEED, t, pi, pr["pl"]) for pi in range(P)]
    else:
        pr = wy.ranksum_problem(genes, vals)
        rows = [rsp.perm_row(SEED, t, pi, pr["valid"], pr["rc"]) for pi in range(P)]
    D = wy.permuted(genes, rows)
    mx = wy.maxs(D, pr["cc"], pr["iv"])
    return pr, wy.r_count(D, pr["d"]), wy.r_fwer(mx, pr["s_obs"]), sd.stepdown(D, pr["cc"], pr["iv"], pr["s_obs"])["r_sd"]


@pytest.mark.parametrize("strata", (False, True))
def test_the_column_is_the_restatements_count(data, strata):
    from scoary_amd import methods as m
    files = STRATA_FILES if strata else RANK_FILES
    seen, below = set(), 0
    for name in files:
        t = ("mic", "growth").index(name.split(".")[0])
        pr, r, rf, rsd = _expected(data, t, strata)
        rows = _rows(data["runs"]["both_strata"][name])
        testable = [g for g in range(G) if pr["iv"][g] > 0]
        assert 5 not in testable and 6 not in testable and sorted(int(row[0][1:]) for row in rows[1:]) == testable
        for row in rows[1:]:
            g = int(row[0][1:])
            assert row[-3] == m._fmt((int(r[g]) + 1.0) / (P + 1.0)), (name, g)
            assert row[-2] == m._fmt((int(rf[g]) + 1.0) / (P + 1.0)), (name, g)
            assert row[-1] == m._fmt((int(rsd[g]) + 1.0) / (P + 1.0)), (name, g)
            seen.add(int(rsd[g]))
        assert (r <= rsd).all() and (rsd <= rf).all()
        below += int((rsd < rf).sum())
        if t == 0:
            assert rsd[7] == rsd[8] == rf[7]                          # the planted gene and its copy: the top group
    assert len(seen) > 5 and min(seen) == 0                           # the planted gene survives the correction


def test_the_files_parse_to_the_engines_values(data):
    """Ranksum_results / VanElteren_results with stepdown=True are what the files were written from: the engine's
    r_sd of the same genes, values and seed."""
    from scoary_amd import methods as m
    eng = m.get_engine()
    gm = eng.pack_dense(data["dense"].astype(np.uint8))
    for strata, files in ((False, RANK_FILES), (True, STRATA_FILES)):
        if strata:
            plan = eng.vanelteren_plan(data["vals"], np.asarray(data["st"], dtype=np.int64))
            got = eng.vanelteren_stepdown(gm, plan, eng.vanelteren(gm, plan), P, SEED)
        else:
            plan = eng.ranksum_plan(data["vals"])
            got = eng.ranksum_stepdown(gm, plan, eng.ranksum(gm, plan), P, SEED)
        rsd = got[2].cpu().numpy()
        for name in files:
            t = ("mic", "growth").index(name.split(".")[0])
            for row in _rows(data["runs"]["sd_strata"][name])[1:]:
                assert row[-1] == m._fmt((int(rsd[t, int(row[0][1:])]) + 1.0) / (P + 1.0)), (name, row[0])
