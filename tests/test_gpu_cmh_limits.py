"""The Cochran-Mantel-Haenszel kernels (spec S10) where they can be wrong without the random cases of
test_gpu_cmh.py noticing: the largest shape the library takes (20 479 isolates, 1024 strata, the most segments the
scratch holds), the region's clamps and ties on purpose, p where erfc underflows, and associate(cmh=True) over
several label batches with every tile width.  The inputs are tests/cmh_cases.py; that they reach these edges is shown
on the CPU in test_cmh_spec.py.  Every expected value is numpy or the plain-Python restatement (cmh_spec.py)."""
import numpy as np
import pytest

import cmh_cases as C
import cmh_spec as S10
from cmh_cases import Case, check_p

pytestmark = pytest.mark.gpu
SEED = 20261018


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    e.set_mfma_route("auto")
    yield e
    e.close()


def check_kernel(eng, c, tiny=0.0):
    """smargins and scounts against numpy, every fp64 output and the region bit for bit against the restatement, p
    by check_p, and the call without scounts against the call with them.  Returns (device outputs, restatement)."""
    out = {k: v.cpu().numpy() for k, v in eng.cmh(c.gm, c.trv, c.mkv, c.sp, scounts=True).items()}
    a, m, k, n = c.recount()
    assert np.array_equal(c.sp.smargins.cpu().numpy(), np.stack([k, n], axis=2))
    assert np.array_equal(out["scounts"], np.stack([a, m], axis=3))
    want = C.restate(a, m, k, n)
    assert np.array_equal(want["a"], (a * (n > 0)[:, None, :]).sum(2))
    assert np.array_equal(out["a"], want["a"])
    for key in ("stat", "e2", "var", "odds"):
        assert np.array_equal(out[key], want[key], equal_nan=True), key
    assert np.array_equal(out["crit"].view(np.uint32), want["crit"])
    dead = want["var"] == 0
    assert np.array_equal(np.isnan(out["stat"]), dead) and (out["p"][dead] == 1.0).all()
    assert np.nanmax(want["stat"], initial=0.0) < 1e4           # the amplification check_p's bound reckons with
    err = check_p(out["p"], want["p"], tiny)
    lean = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    assert "scounts" not in lean
    for key in ("stat", "p", "odds", "e2", "var", "a", "crit"):
        assert np.array_equal(lean[key].cpu().numpy(), out[key], equal_nan=True), key
    return out, want, err


@pytest.mark.parametrize("name", list(C.LIMIT_GENES))
def test_limit_shapes_against_numpy_and_the_restatement(eng, name):
    """N = 20 479 (word indices to 639), S = 1024, T = 5 (two trait blocks, three surplus slots in the second):
    'interleaved' has one segment per isolate, 'blocked' runs of up to 32 members with boundaries inside words and
    indices without members, 'two_level' 16-member runs across the segment builder's 20-member chunks and more than
    one block of genes."""
    assert (int(eng.lib.scoary_perm_strata_max_isolates()), int(eng.lib.scoary_perm_max_strata())) == \
        (C.LIMIT_N, C.LIMIT_S) == (20479, 1024)
    genes, traits, strata = C.limit_case(name)
    if name == "interleaved":            # no two members of a stratum share a word: N segments
        assert len(np.unique(strata * 1024 + np.arange(C.LIMIT_N) // 32)) == C.LIMIT_N
    c = Case(eng, genes, traits, strata, S=C.LIMIT_S)
    assert (c.T, c.N, c.S) == (5, C.LIMIT_N, C.LIMIT_S) and (c.traits == 2).any()
    _out, want, _err = check_kernel(eng, c, tiny=C.P_NORMAL)
    dead = want["var"] == 0
    assert dead.any() and not dead.all()                       # genes 1 and 2 are in no / every isolate
    assert (want["crit"][..., 1] > 0).any()


def test_the_regions_clamps_and_ties_on_the_device(eng):
    """The constructed genes of cmh_cases.edge_case(): no informative stratum, A = E, half a count from E, lo < 0
    and hi > K before their clamps, an exact mirror tie, odds = inf, and strata of 0 and 1 valid isolates made by
    the mask (test_cmh_spec.py asserts each from the restatement and Fractions)."""
    genes, traits, strata, names = C.edge_case()
    c = Case(eng, genes, traits, strata, S=len(C.EDGE_NK))
    out, want, _err = check_kernel(eng, c)
    g = {name: i for i, name in enumerate(names)}
    crit = out["crit"].view(np.uint32)
    K = sum(k for _n, k in C.EDGE_NK)
    # what the restatement gave is asserted bit for bit above; the landmarks once more on the device's own output
    assert crit[0, g["lo_clamp"]].tolist() == [0, out["a"][0, g["lo_clamp"]]]
    assert crit[0, g["hi_clamp"]].sum() == K + 1
    assert crit[0, g["a_equals_e"]].tolist() == [0, 0] and out["stat"][0, g["a_equals_e"]] == 0.0
    assert crit[0, g["inside_cc"]].tolist() == [0, 0] and out["stat"][0, g["inside_cc"]] == 0.0
    assert out["odds"][0, g["odds_inf"]] == np.inf and np.isnan(out["stat"][0, g["dead"]])


def test_p_at_large_statistics(eng):
    """Statistics from 60 to 6000: p down to the smallest normal doubles within 1e-10 relative of math.erfc,
    subnormals and zeros within 1e-12 absolute and not negative.
    Measured on the MI355X: see profiles/cmh_tests.txt."""
    genes, traits, strata = C.graded_case()
    c = Case(eng, genes, traits, strata, S=4)
    out, want, (err, rel, worst) = check_kernel(eng, c, tiny=C.P_NORMAL)
    p, stat = want["p"], want["stat"]
    tiny = p < C.P_NORMAL
    assert tiny.any() and (p[tiny] > 0).any() and (p[tiny] == 0).any() and ((p >= C.P_NORMAL) & (p < 1e-200)).any()
    sub = tiny & (p > 0)
    print("cmh p at large statistics: max relative error %.3e at stat %.2f (p %.3e); %d normal p below 1e-200, "
          "%d subnormal (device: %d nonzero, largest |dp| %.3e), %d zero (device: %d zero)"
          % (rel, stat[worst], p[worst], ((p >= C.P_NORMAL) & (p < 1e-200)).sum(), sub.sum(),
             (out["p"][sub] > 0).sum(), np.abs(out["p"][sub] - p[sub]).max(), (p == 0).sum(),
             (out["p"][p == 0] == 0).sum()))
    assert (out["p"][stat > 3000] == 0).all()                  # erfc(> 38) is no double but 0


def host_r(a_perm, crit):
    """The count the permutation kernels make, [T, G]: permutations with (uint32)(a' - base) >= span."""
    c = crit.astype(np.int64)
    return S10.in_region((c[:, None, :, 0], c[:, None, :, 1]), a_perm).sum(1).astype(np.uint32)


@pytest.mark.parametrize("name", list(C.BATCH_CASES))
def test_associate_cmh_over_several_label_batches(eng, monkeypatch, name):
    """r_cmh and r of a step whose labels come in several batches (the last one ragged) equal the one-batch step
    and a host count on the downloaded labels -- r_cmh with the restatement's regions, not the device's."""
    genes, traits, strata, S, P, batch, tw = C.batch_case(name)
    c = Case(eng, genes, traits, strata, S=S)
    lists = tw is not None
    if lists:
        assert eng.list_params(c.N)[0] == tw                   # the tile kernel this case is for
        eng.build_lists(c.gm)

    def step(permutations, cmh=True):
        res = eng.associate(c.gm, c.trv, c.mkv, permutations=permutations, seed=SEED, use_lists=lists, strata=c.sp,
                            cmh=cmh)
        return {k: v.cpu().numpy() for k, v in res.items()}

    one = step(P)                                              # the engine's own batch: all P at once
    if lists:
        assert eng.list_batch(c.T, c.N, P, c.G) >= P
        monkeypatch.setattr(eng, "list_batch", lambda *a, **k: batch)
    else:
        assert eng.perm_batch(c.T, c.N, P) >= P
        monkeypatch.setattr(eng, "perm_batch", lambda *a, **k: batch)
    assert -(-P // batch) >= 2 and P % batch
    res = step(P)
    plain = step(P, cmh=False)
    first = step(batch)
    monkeypatch.undo()

    a, m, k, n = c.recount()
    want = C.restate(a, m, k, n)
    assert np.array_equal(res["cmh_crit"].view(np.uint32), want["crit"])
    bits = c.label_rows(eng, P, SEED)
    a_perm = C.pooled_counts(bits, c.genes)
    want_cmh, want_fisher = host_r(a_perm, want["crit"]), host_r(a_perm, res["crit"].view(np.uint32))
    r_cmh, r = res["r_cmh"].view(np.uint32), res["r"].view(np.uint32)
    assert np.array_equal(r_cmh, want_cmh) and np.array_equal(r, want_fisher)
    assert np.array_equal(one["r_cmh"].view(np.uint32), r_cmh) and np.array_equal(one["r"].view(np.uint32), r)
    assert (r_cmh < P).any() and (r_cmh > 0).any()
    # the later batches were counted, and into the right counter
    assert np.array_equal(first["r_cmh"].view(np.uint32), host_r(a_perm[:, :batch], want["crit"]))
    assert (first["r_cmh"].view(np.uint32) != r_cmh).any() and (first["r"].view(np.uint32) != r).any()
    assert "r_cmh" not in plain and "cmh_p" not in plain
    for key in ("r", "p", "counts", "crit"):
        assert np.array_equal(plain[key], res[key]), key
    # the regions counted against are the exact rule on every pooled count that occurred (S10's slack at a near tie)
    for t, g in C.subsample_pairs(c.T, c.G):
        occurred = np.unique(a_perm[t, :, g])
        assert C.exact_rule_mismatches(C.tables(a, m, k, n, t, g), tuple(int(x) for x in want["crit"][t, g]),
                                       occurred) == [], (t, g)
