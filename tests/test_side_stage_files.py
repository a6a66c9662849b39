"""The files and refusals of the side stages (--quantitative, --quantitative-strata, --categorical,
--categorical-strata), byte for byte: the four Store*Results on hand-built result dictionaries and the two trait-file
readers on malformed files, against text recorded from the writers and readers as they stood before they were given
one file loop and one reader (tests/golden/side_stage/expected.json).  No GPU and no engine: the stores only format.

    python tests/test_side_stage_files.py --record      rewrites the fixture from the code in the tree"""
import json
import os
import sys

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "side_stage", "expected.json")
INF = float("inf")


class Table:
    """Three genes in the gene table's order; the second id carries the Roary name cells itself."""
    ids = ["geneA", "grp7_|_nm7_|_an annotation; with a delimiter", "geneC"]
    nugn = ["nuA", "", "nuC"]
    annotation = ["annotation A", "", "annotation, C"]
    strains = []


OPTIONAL = dict(r=np.array([4, 0, 19]), permutations=19, r_fwer=np.array([9, 1, 19]), r_sd=np.array([9, 3, 19]),
                shift=np.array([0.5, -1.25, 0.0]), shift_lower=np.array([-INF, -2.0, -0.5]),
                shift_upper=np.array([1.5, -0.75, INF]))
P = np.array([0.04, 0.001, 0.04])                       # a tie: the file order decides
M = np.array([3, 6, 5])


def _base(store):
    if store in ("StoreRanksumResults", "StoreVanElterenResults"):
        return dict(n=11, m=M, auc=np.array([0.75, 0.9375, 0.25]), p=P)
    common = dict(classes=["a", "b;c", "d"], n=11, m=M, a=np.array([[1, 2, 0], [4, 1, 1], [0, 2, 3]]), p=P)
    if store == "StoreCategoricalResults":
        return dict(common, nk=np.array([5, 4, 2]), df=2, x2=np.array([4.25, 13.5, 4.25]),
                    v=np.array([0.625, 0.875, 0.625]))
    return dict(common, e=np.array([[1.5, 1.0, 0.5], [2.75, 2.25, 1.0], [2.5, 0.0, 2.5]]),
                q=np.array([4.25, 13.5, 4.25]), df=np.array([2, 2, 1]))


STORES = {"StoreRanksumResults": ".ranksum.results.csv", "StoreVanElterenResults": ".vanelteren.results.csv",
          "StoreCategoricalResults": ".categorical.results.csv", "StoreGcmhResults": ".gcmh.results.csv"}
# (setting, max_hits, delimiter): every optional key, none of them, no testable gene
SETTINGS = (("full", None, ","), ("full", 1, ";"), ("full", 0, ","), ("none", None, ";"), ("none", 1, ","),
            ("empty", None, ","), ("empty", 1, ";"))


def _results(store, setting):
    res = dict(_base(store), testable=np.array([setting != "empty"] * 3))
    if setting != "none":
        res.update(OPTIONAL)
    return {"trait one": res, "t2": dict(res, testable=np.array([False, setting != "empty", False]))}


def _store(m, store, setting, max_hits, delimiter, outdir):
    files = getattr(m, store)(_results(store, setting), Table, max_hits, outdir, time="_T", delimiter=delimiter)
    assert files == [outdir + name + "_T" + STORES[store] for name in ("trait one", "t2")]
    return [open(f).read() for f in files]


HEAD = {"quantitative": "Name,length,weight\n", "categorical": "Name,host,site\n"}
GOOD = {"quantitative": "s1,1.5,2\ns2,NA,-3e2\nunknown,7,7\n\ns4,.,0.25\n", "categorical": "s1,cow,x\ns2,NA,y z\nunknown,pig,x\n\ns4,-,inf\n"}
MALFORMED = {"no trait column": "Name\ns1\n", "empty file": "", "duplicate trait": "Name,w,w\ns1,1,2\n",
             "duplicate isolate": "%ss1,1,2\ns2,3,4\ns1,5,6\n", "short row": "%ss1,1,2\ns2,3\n",
             "short row of an isolate the analysis does not hold": "%sother,1\n"}
NON_FINITE = {"inf": "%ss1,1,inf\n", "nan": "%ss1,nan,2\n", "word": "%ss1,1,2\ns2,heavy,4\n"}
STRAINS = ["s1", "s2", "s3", "s4"]


def _reader_cases(what):
    cases = dict(MALFORMED, **(NON_FINITE if what == "quantitative" else {}))
    return {k: (v % HEAD[what] if "%s" in v else v) for k, v in cases.items()}


def _refusal(m, what, text, delimiter=","):
    with open(what[0] + ".csv", "w") as f:              # a relative path: the messages name it
        f.write(text)
    with pytest.raises(SystemExit) as e:
        getattr(m, "read_%s_file" % what)(what[0] + ".csv", delimiter, STRAINS)
    return str(e.value)


def _everything(m, outdir):
    out = {}
    for store in STORES:
        for setting, max_hits, delimiter in SETTINGS:
            out["%s %s max_hits=%s %s" % (store, setting, max_hits, delimiter)] = _store(m, store, setting, max_hits,
                                                                                        delimiter, outdir)
    for what in HEAD:
        for case, text in _reader_cases(what).items():
            out["read_%s_file %s" % (what, case)] = _refusal(m, what, text)
    return out


@pytest.fixture()
def methods(monkeypatch, tmp_path):
    from scoary_amd import methods as m
    monkeypatch.setattr(m, "_as_table", lambda g: g)
    monkeypatch.chdir(tmp_path)
    return m


@pytest.fixture(scope="module")
def expected():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("store", sorted(STORES))
def test_the_stores_write_the_recorded_bytes(methods, expected, tmp_path, store):
    out = str(tmp_path) + os.sep
    for setting, max_hits, delimiter in SETTINGS:
        key = "%s %s max_hits=%s %s" % (store, setting, max_hits, delimiter)
        got = _store(methods, store, setting, max_hits, delimiter, out)
        assert got == expected[key], key
        lines = got[0].splitlines()
        assert len(lines) == 1 + (0 if setting == "empty" else 3 if max_hits is None else max_hits), key
        assert ("Empirical_p" in lines[0]) == (setting != "none"), key
    # the fixture holds what it is read for: both orders of the tie, the name cells of the id, an infinite limit
    full = expected["%s full max_hits=None ," % store][0].splitlines()
    assert [l.split(",")[0] for l in full[1:]] == ['"grp7"', '"geneA"', '"geneC"']
    assert full[1].startswith('"grp7","nm7","an annotation; with a delimiter",')
    assert ('"-inf"' in full[2]) == (store in ("StoreRanksumResults", "StoreVanElterenResults"))


@pytest.mark.parametrize("what", sorted(HEAD))
def test_the_readers_refuse_with_the_recorded_words(methods, expected, what):
    cases = _reader_cases(what)
    assert len(cases) == (9 if what == "quantitative" else 6)
    for case, text in cases.items():
        got = _refusal(methods, what, text)
        assert got == expected["read_%s_file %s" % (what, case)], case
        assert ("The %s traits file %s.csv" % (what, what[0]) in got
                or got.startswith("Please check that the %s traits file %s.csv" % (what, what[0]))), case


def test_the_readers_read(methods):
    for what in HEAD:
        for delimiter in (",", ";"):
            with open("good.csv", "w") as f:
                f.write((HEAD[what] + GOOD[what]).replace(",", delimiter))
            names, rows = getattr(methods, "read_%s_file" % what)("good.csv", delimiter, STRAINS)
            if what == "quantitative":
                assert names == ["length", "weight"]
                assert np.array_equal(rows, np.array([[1.5, np.nan, np.nan, np.nan], [2.0, -300.0, np.nan, 0.25]]),
                                      equal_nan=True) and rows.dtype == np.float64
            else:
                assert names == ["host", "site"]
                assert rows == [["cow", None, None, None], ["x", "y z", None, "inf"]]


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from scoary_amd import methods as _m
    _m._as_table = lambda g: g
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        recorded = _everything(_m, tmp + os.sep)
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
