"""The randomised cross-checks of the stratified statistics (tests/strata_stress_cases.py) under `pytest -m gpu`: one
test per family, a fixed number of cases each (strata_stress_cases.POOLS) and no wall-clock budget -- a test that stops
early hides cases.  tests/test_strata_stress_corpus.py shows on the CPU what these corpora reach; the seconds every
test takes are in profiles/strata_stress.txt."""
import pytest

import strata_stress_cases as ssc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _run(eng, family):
    cases, done, bad = ssc.POOLS[family]["cases"], 0, []
    for case in range(cases):
        ok, what = ssc.FAMILIES[family](eng, case)
        done += 1
        print(("ok   " if ok else "FAIL ") + what)
        if not ok:
            bad.append(what)
    assert done == cases
    assert not bad, "\n".join(["%d of %d cases fail:" % (len(bad), cases)] + bad)


def test_stress_stratified_label_rows_and_tiles(eng):
    _run(eng, "A")


def test_stress_cmh_and_the_exact_test_family(eng):
    ssc.B_TALLY.update(pairs=0, ties=0)
    _run(eng, "B")
    pairs, ties = ssc.B_TALLY["pairs"], ssc.B_TALLY["ties"]
    print("family B: %d pairs, %d near ties left out of the p comparison" % (pairs, ties))
    assert pairs >= 100 and ties <= 0.01 * pairs


def test_stress_counts_under_stratified_permutations(eng):
    _run(eng, "C")


def test_stress_westfall_young_over_three_kinds_of_table(eng):
    _run(eng, "D")


def test_stress_matrix_core_routing_under_strata(eng):
    _run(eng, "E")
