"""--quantitative-shift through main(): test_gpu_rank_wy_cli's small synthetic data set (60 genes x 40 isolates, two
measured traits, four strata), run with the flag and without it, without permutations and with --permute 100
--quantitative-fwer-stepdown, with --quantitative-strata and at another level.  The three cells of every row are
_fmt of the restatement's values (rank_shift_spec.py); with the three columns cut out the files of a run with the
flag are the files of the run without it, byte for byte; without the flag nothing names the shift; the van Elteren
file and the binary trait's file do not change."""
import csv
import io

import numpy as np
import pytest

import rank_shift_spec as spec
from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
G, N, P, SEED = 60, 40, 100, 4242
RANK_FILES = ["growth.ranksum.results.csv", "mic.ranksum.results.csv"]
STRATA_FILES = ["growth.vanelteren.results.csv", "mic.vanelteren.results.csv"]
COLUMNS = ["Rank_sum_shift", "Rank_sum_shift_lower", "Rank_sum_shift_upper"]
FLAG = "--quantitative-shift"


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    rng = np.random.default_rng(60)
    d = tmp_path_factory.mktemp("rank_shift_cli")
    dense = rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))
    dense[5], dense[6] = False, True
    mic = np.round(np.exp2(rng.integers(-3, 4, N).astype(float)), 3)          # MIC-like: heavy ties
    dense[7] = rng.random(N) < 0.5
    mic[dense[7]] += 100.0                                                    # gene 7 carries the phenotype
    dense[9] = False
    dense[9, 11] = True                                                       # one carrier: no interval at 95 %
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
    common = ["-g", str(d / "g.csv"), "-t", str(d / "t.csv"), "--no_pairwise", "--seed", str(SEED), "-p", "1.0",
              "--quantitative", str(d / "q.csv")]
    strata = ["--quantitative-strata", str(d / "strata.csv")]
    perms = ["-e", str(P), "--quantitative-fwer-stepdown"]
    runs = dict(shift=run_cli(common + strata + [FLAG], d / "out_s"),
                plain=run_cli(common + strata, d / "out_p"),
                shift_perm=run_cli(common + strata + perms + [FLAG], d / "out_sp"),
                plain_perm=run_cli(common + strata + perms, d / "out_pp"),
                shift_half=run_cli(common + [FLAG, "--quantitative-shift-level", "0.5"], d / "out_h"))
    (d / "big.csv").write_text("Name,mic\n" + "".join("%s,%s\n" % (iso[i], "2e150" if i == 4 else "1.0")
                                                      for i in range(N)))
    return dict(dense=dense.astype(np.int64), vals=vals, runs=runs, dir=d, common=common)


def _rows(text):
    assert all(line.startswith('"') and line.endswith('"') for line in text.splitlines())
    return list(csv.reader(io.StringIO(text)))


def _without_the_columns(text):
    rows = _rows(text)
    at = rows[0].index(COLUMNS[0])
    assert rows[0][at:at + 3] == COLUMNS and rows[0][at - 1] == "Benjamini_H_p"
    return "".join(",".join('"%s"' % c for c in row[:at] + row[at + 3:]) + "\n" for row in rows)


def test_without_the_flag_nothing_names_the_shift(data):
    runs = data["runs"]
    for run in ("plain", "plain_perm"):
        assert sorted(runs[run]) == sorted(["bin.results.csv"] + RANK_FILES + STRATA_FILES)
        assert not any("shift" in text for text in runs[run].values())
    assert _rows(runs["plain"][RANK_FILES[0]])[0][-1] == "Benjamini_H_p"
    assert _rows(runs["plain_perm"][RANK_FILES[0]])[0][-2:] == ["Empirical_p", "Westfall_Young_stepdown_p"]


@pytest.mark.parametrize("with_flag, without", (("shift", "plain"), ("shift_perm", "plain_perm")))
def test_with_the_columns_cut_out_the_files_are_the_files_without_the_flag(data, with_flag, without):
    got, want = data["runs"][with_flag], data["runs"][without]
    assert sorted(got) == sorted(want)
    for name in RANK_FILES:
        assert _without_the_columns(got[name]) == want[name]                  # byte for byte
        assert len(_rows(got[name])) > 20
    for name in STRATA_FILES + ["bin.results.csv"]:                           # the flag changes no other file
        assert got[name] == want[name]
    head = _rows(got[RANK_FILES[0]])[0]
    if with_flag == "shift_perm":                                             # the permutation columns stay last
        assert head[-5:] == COLUMNS + ["Empirical_p", "Westfall_Young_stepdown_p"]
    else:
        assert head[-3:] == COLUMNS


@pytest.mark.parametrize("run, level", (("shift", 0.95), ("shift_perm", 0.95), ("shift_half", 0.5)))
def test_the_cells_are_the_restatements_values(data, run, level):
    from scoary_amd import methods as m
    infinite = finite = 0
    for name in RANK_FILES:
        t = ("mic", "growth").index(name.split(".")[0])
        rows = _rows(data["runs"][run][name])
        at = rows[0].index(COLUMNS[0])
        seen = []
        for row in rows[1:]:
            g = int(row[0][1:])
            shift, lower, upper, _ca, _raw = spec.shift_spec(data["vals"][t], data["dense"][g], level)
            assert row[at:at + 3] == [m._fmt(shift), m._fmt(lower), m._fmt(upper)], (name, g)
            assert float(row[at + 1]) <= float(row[at]) <= float(row[at + 2])
            infinite += row[at + 1] == "-inf" and row[at + 2] == "inf"
            finite += "inf" not in row[at + 1] + row[at + 2]
            seen.append(g)
        assert 5 not in seen and 6 not in seen and 9 in seen and 7 in seen
        if t == 0:                                                            # the planted 100 units are found
            row7 = next(row for row in rows[1:] if row[0] == "g007")
            assert 95 < float(row7[at]) < 105 and float(row7[at + 1]) > 90
    assert finite > 40 and (infinite > 0) == (level == 0.95)                  # gene 9: one carrier


def test_a_value_past_1e150_is_refused_with_the_flag_only(data):
    from scoary_amd import methods as m
    import sys
    d, common = data["dir"], list(data["common"])
    common[common.index("--quantitative") + 1] = str(d / "big.csv")
    out = run_cli(common, d / "out_big")                                      # the rank-sum test ranks it
    assert "mic.ranksum.results.csv" in out
    old = sys.argv
    sys.argv = ["scoary"] + common + [FLAG, "-o", str(d / "out_big2"), "--no-time"]
    try:
        with pytest.raises(SystemExit) as e:
            m.main()
    finally:
        sys.argv = old
    assert e.value.code == m.RANK_SHIFT_TEXT["magnitude"]
