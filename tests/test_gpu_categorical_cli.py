"""--categorical FILE through main(): a 40-isolate table with a 3-class and a 2-class trait, run with the flag (with
--permute 60 and without permutations) and without it -- the new files, their columns, their row order and every cell
against the engine's calls and the restatement (categorical_spec.py), and every ordinary result file byte for byte the
same in both runs."""
import csv
import io
import os

import numpy as np
import pytest

import categorical_spec as cs
from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu
G, N, P, SEED = 75, 40, 60, 777
COLUMNS = ["Gene", "Non-unique Gene name", "Annotation", "Number_with_gene", "Number_without_gene", "Carriers_by_class",
           "Most_enriched_class", "Chi2", "Chi2_df", "Cramers_V", "Chi2_p", "Bonferroni_p", "Benjamini_H_p"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    rng = np.random.default_rng(44)
    d = tmp_path_factory.mktemp("categorical_cli")
    dense = rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))
    dense[5], dense[6] = False, True
    host = [["pig", "cattle", "human"][k] for k in rng.integers(0, 3, N)]     # sorted: cattle, human, pig
    source = [["blood", "Faeces"][k] for k in rng.integers(0, 2, N)]          # sorted as strings: Faeces, blood
    dense[7] = [h == "pig" for h in host]                                    # gene 7 is the class pig: X2 = n
    for i in (3, 14, 25):
        host[i] = None
    source[8] = None
    iso = ["s%02d" % i for i in range(N)]
    meta = ["Gene", "Non-unique Gene name", "Annotation", "No. isolates", "No. sequences",
            "Avg sequences per isolate", "Genome Fragment", "Order within Fragment",
            "Accessory Fragment", "Accessory Order with Fragment", "QC", "Min group size nuc",
            "Max group size nuc", "Avg group size nuc"]
    cells = np.where(dense, "x", "")
    (d / "g.csv").write_text(",".join(meta + iso) + "\n" + "".join(
        "g%03d,nu%d,\"an, %d\",%s,%s\n" % (g, g, g, ",".join(["1"] * 11), ",".join(cells[g])) for g in range(G)))
    (d / "t.csv").write_text(",bin\n" + "".join("%s,%d\n" % (iso[i], i % 3 == 0) for i in range(N)))
    crows = []
    for i in range(N):
        if i == 9:
            continue                                                          # absent from the file: missing
        crows.append("%s,%s,%s\n" % (iso[i], host[i] or "NA", source[i] or "-"))
    (d / "c.csv").write_text("Name,host,source\n" + "".join(crows) + "other,llama,soil\n")
    host[9] = source[9] = None
    common = ["-g", str(d / "g.csv"), "-t", str(d / "t.csv"), "--no_pairwise", "--seed", str(SEED), "-p", "1.0"]
    flag = ["--categorical", str(d / "c.csv")]
    return dict(dense=dense.astype(np.uint8), labels=[host, source], dir=d,
                with_c=run_cli(common + ["-e", str(P)] + flag, d / "out_c"),
                without=run_cli(common + ["-e", str(P)], d / "out_plain"),
                no_perm=run_cli(common + flag + ["-m", "7"], d / "out_noperm"))


def test_ordinary_result_files_are_byte_identical(data):
    assert sorted(data["without"]) == ["bin.results.csv"]
    assert sorted(data["with_c"]) == ["bin.results.csv", "host.categorical.results.csv",
                                      "source.categorical.results.csv"]
    assert data["with_c"]["bin.results.csv"] == data["without"]["bin.results.csv"]
    assert len(data["without"]["bin.results.csv"].splitlines()) > 10


def test_categorical_files_hold_what_the_engine_returns_and_the_restatement(data):
    from scoary_amd import methods as m
    eng = m.get_engine()
    gm = eng.pack_dense(data["dense"])
    spec = [cs.codes_of(row) for row in data["labels"]]
    assert [s[0] for s in spec] == [["cattle", "human", "pig"], ["Faeces", "blood"]]
    codes = np.array([s[1] for s in spec])
    plan = eng.categorical_plan(codes)
    res = eng.categorical(gm, plan)
    r = eng.categorical_permute(gm, plan, res["a"], P, SEED).cpu().numpy()
    a, mm, x2, p, v = (res[k].cpu().numpy() for k in ("a", "m", "x2", "p", "v"))
    for t, name in enumerate(("host", "source")):
        classes, row = spec[t]
        K = len(classes)
        nk = cs.sizes(row, K)
        n = sum(nk)
        assert n == (N - 4, N - 2)[t]
        rows_spec = [cs.perm_row(SEED, t, pi, row) for pi in range(P)]
        text = data["with_c"][name + ".categorical.results.csv"]
        assert all(line.startswith('"') and line.endswith('"') for line in text.splitlines())
        rows = list(csv.reader(io.StringIO(text)))
        assert rows[0] == COLUMNS + ["Empirical_p"]
        testable = [g for g in range(G) if 0 < mm[t, g] < n]
        assert 5 not in testable and 6 not in testable and len(rows) - 1 == len(testable) >= G - 6
        order = sorted(testable, key=lambda g: (p[t, g], g))             # ascending p, ties in file order
        assert [line[0] for line in rows[1:]] == ["g%03d" % g for g in order]
        bonf, bh = m.bonferroni_bh(p[t, testable], len(testable))
        for line in rows[1:]:
            g = int(line[0][1:])
            k = testable.index(g)
            gene = data["dense"][g].tolist()
            tab = cs.table(gene, row, K)
            ok, sx2, df, sp, sv = cs.statistic(tab, nk)
            assert ok and a[t, g, :K].tolist() == tab and x2[t, g] == sx2
            assert abs(p[t, g] - sp) <= 1e-10 * sp and abs(v[t, g] - sv) <= 2.0 ** -52 * sv
            assert int(r[t, g]) == cs.r_count(gene, rows_spec, row, K)
            assert line[1:3] == ["nu%d" % g, "an, %d" % g]
            assert line[3:] == [m._fmt(sum(tab)), m._fmt(n - sum(tab)),
                                "|".join("%s=%d" % (c, x) for c, x in zip(classes, tab)),
                                classes[cs.most_enriched(tab, nk)], m._fmt(sx2), str(K - 1), m._fmt(v[t, g]),
                                m._fmt(p[t, g]), m._fmt(bonf[k]), m._fmt(bh[k]),
                                m._fmt((int(r[t, g]) + 1.0) / (P + 1.0))]
    top = list(csv.reader(io.StringIO(data["with_c"]["host.categorical.results.csv"])))[1]
    assert top[0] == "g007" and top[6] == "pig" and float(top[7]) == pytest.approx(N - 4, rel=1e-12)
    assert float(top[9]) == pytest.approx(1.0, abs=1e-12)


def test_max_hits_and_no_permutations(data):
    whole = list(csv.reader(io.StringIO(data["with_c"]["host.categorical.results.csv"])))
    got = list(csv.reader(io.StringIO(data["no_perm"]["host.categorical.results.csv"])))
    assert got[0] == COLUMNS and len(got) == 8                               # no Empirical_p, seven rows
    assert got[1:] == [row[:-1] for row in whole[1:8]]
    log = open(os.path.join(str(data["dir"] / "out_noperm"), "scoary.log")).read()
    assert "Chi-square test of host: %d isolates with a label in 3 classes" % (N - 4) in log
