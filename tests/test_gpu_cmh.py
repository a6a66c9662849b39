"""The Cochran-Mantel-Haenszel kernel (spec S10) and associate(cmh=True): per-stratum counts against numpy, every
fp64 result bit for bit against the plain-Python restatement (tests/cmh_spec.py), the exceedance counts against a
host recount from the downloaded stratified labels."""
import ctypes

import numpy as np
import pytest

import cmh_spec as S10
from cmh_cases import Case, check_cmh, check_p, random_genes_traits, restate

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


def build_case(eng, name):
    if name == "interleaved":            # random strata, 257 isolates = 9 words: a quad tail, missing values in trait 2
        genes, traits, rng = random_genes_traits(300, 257, 3, 4)
        return Case(eng, genes, traits, rng.integers(0, 4, 257), S=4)
    if name == "singletons":             # strata of one isolate, strata emptied by the mask, a stratum without members
        genes, traits, rng = random_genes_traits(130, 129, 2, 40)
        strata = rng.integers(0, 36, 129)
        strata[5], strata[77], strata[[9, 10]] = 36, 37, 38
        traits[1, [9, 10, 77]] = 2                                              # 38 and 37 are empty for trait 1
        return Case(eng, genes, traits, strata, S=40)
    if name == "contiguous":             # boundaries inside words; more isolates than the matrix-core kernel takes
        genes, traits, rng = random_genes_traits(200, 2100, 2, 7)
        bounds = np.array([13, 300, 301, 1000, 1555, 2047])
        return Case(eng, genes, traits, np.searchsorted(bounds, np.arange(2100), side="right"), S=7)
    if name == "traits33":               # more traits than one pass of the counts kernel (32)
        genes, traits, rng = random_genes_traits(64, 96, 33, 3)
        return Case(eng, genes, traits, rng.integers(0, 3, 96), S=3)
    assert name == "one_stratum"
    genes, traits, rng = random_genes_traits(300, 257, 3, 1)
    return Case(eng, genes, traits, np.zeros(257, dtype=np.int64), S=1)


@pytest.mark.parametrize("name", ["interleaved", "singletons", "contiguous", "traits33", "one_stratum"])
def test_kernel_against_numpy_and_the_restatement(eng, name):
    c = build_case(eng, name)
    out = {k: v.cpu().numpy() for k, v in eng.cmh(c.gm, c.trv, c.mkv, c.sp, scounts=True).items()}
    a, m, k, n = c.recount()
    assert np.array_equal(c.sp.smargins.cpu().numpy(), np.stack([k, n], axis=2))
    assert np.array_equal(out["scounts"], np.stack([a, m], axis=3))
    assert np.array_equal(out["a"], (a * (n > 0)[:, None, :]).sum(2))
    dead = check_cmh(out, restate(a, m, k, n))
    assert dead.any() and not dead.all()                       # genes 1 and 2 are in no / every isolate
    # without the per-stratum tables the results are the same
    lean = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    assert "scounts" not in lean
    for key in ("stat", "p", "odds", "e2", "var", "a", "crit"):
        assert np.array_equal(lean[key].cpu().numpy(), out[key], equal_nan=True), key


def test_ucb_admissions_on_the_device(eng):
    """The six departments as strata of 4526 isolates, admission as the trait, sex as the one gene."""
    UCB, tables_abcd = S10.UCB, S10.tables_abcd
    gene, trait, strata = [], [], []
    for s, (a, b, c, d) in enumerate(UCB.values()):
        gene += [1] * a + [0] * b + [1] * c + [0] * d
        trait += [1] * (a + b) + [0] * (c + d)
        strata += [s] * (a + b + c + d)
    assert len(gene) == 4526
    c = Case(eng, np.array([gene]), np.array([trait]), np.array(strata), S=6)
    out = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    want = S10.cmh(tables_abcd(UCB.values()))
    assert out["stat"].item() == want["stat"] and out["odds"].item() == want["odds"]
    assert abs(want["stat"] - 1.4269462285866712) <= 1e-12 * 1.4269462285866712
    check_p(np.array([out["p"].item()]), np.array([0.23226346281705096]))
    assert tuple(out["crit"].cpu().numpy().view(np.uint32)[0, 0]) == want["crit"]


def want_r(a_perm, crit):
    c = crit.cpu().numpy().view(np.uint32).astype(np.int64)
    return (((a_perm - c[:, None, :, 0]) & 0xffffffff) >= c[:, None, :, 1]).sum(1).astype(np.uint32)


def check_associate(eng, c, P, use_lists):
    res = eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=SEED, use_lists=use_lists, strata=c.sp, cmh=True)
    _bits, a_perm = c.labels(eng, P, SEED)
    got = res["r_cmh"].cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want_r(a_perm, res["cmh_crit"]))
    assert (got < P).any() and (got > 0).any()
    alone = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    for key in ("stat", "p", "odds", "crit"):
        assert np.array_equal(res["cmh_" + key].cpu().numpy(), alone[key].cpu().numpy(), equal_nan=True)
    plain = eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=SEED, use_lists=use_lists, strata=c.sp)
    assert "r_cmh" not in plain and "cmh_p" not in plain
    for key in ("r", "p", "counts", "crit"):
        assert np.array_equal(plain[key].cpu().numpy(), res[key].cpu().numpy()), key
    assert np.array_equal(res["r"].cpu().numpy().view(np.uint32), want_r(a_perm, res["crit"]))


@pytest.mark.parametrize("use_lists", [False, True], ids=["dense", "lists"])
def test_associate_counts_the_cmh_region_on_the_same_labels(eng, use_lists):
    c = build_case(eng, "interleaved")
    if use_lists:
        eng.build_lists(c.gm)
    check_associate(eng, c, 320, use_lists)


def test_associate_cmh_with_the_matrix_core_kernel(eng):
    genes, traits, rng = random_genes_traits(512, 600, 2, 5, dense_genes=True)
    c = Case(eng, genes, traits, rng.integers(0, 5, 600), S=5)
    eng.set_mfma_route("all")
    try:
        eng.build_lists(c.gm)
        if eng.mfma_split(c.gm, c.T, 320) <= 0:
            pytest.skip("the matrix-core kernel takes no slot of this shape (mfma_split = 0)")
        check_associate(eng, c, 320, True)
    finally:
        eng.set_mfma_route("auto")


def test_associate_cmh_without_permutations_and_its_refusals(eng):
    c = build_case(eng, "one_stratum")
    res = eng.associate(c.gm, c.trv, c.mkv, strata=c.sp, cmh=True)
    assert res["r"] is None and "r_cmh" not in res
    alone = eng.cmh(c.gm, c.trv, c.mkv, c.sp)
    assert np.array_equal(res["cmh_p"].cpu().numpy(), alone["p"].cpu().numpy())
    with pytest.raises(ValueError, match="strata"):
        eng.associate(c.gm, c.trv, c.mkv, cmh=True)
    # the library's own limits: more strata than the strata plan takes
    z = ctypes.c_void_p(8)                                    # never dereferenced: the sizes are refused first
    rc = eng.lib.scoary_cmh(eng.h, *([z] * 7), 10, 1, 100, eng.strata_max()[0] + 1, *([z] * 9), None)
    assert rc == -3 and b"strata" in eng.lib.scoary_last_error(eng.h)
    rc = eng.lib.scoary_cmh(eng.h, *([z] * 7), 10, 1, eng.strata_max()[1] + 1, 2, *([z] * 9), None)
    assert rc == -3 and b"isolates" in eng.lib.scoary_last_error(eng.h)


def test_a_lineage_marker_is_confounded_and_a_within_stratum_signal_is_not(eng):
    rng = np.random.default_rng(3)
    G, N, P, S = 200, 300, 256, 6
    strata = rng.integers(0, S, N)
    lineage = (strata < 3).astype(np.uint8)
    genes = (rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))).astype(np.uint8)
    genes[0] = np.where(rng.random(N) < 0.95, lineage, 1 - lineage)              # the lineage marker
    # trait 0: constant inside every stratum; trait 1: follows gene 5 inside every stratum, no lineage effect
    signal = np.where(rng.random(N) < 0.8, genes[5], rng.random(N) < 0.5).astype(np.uint8)
    c = Case(eng, genes, np.stack([lineage, signal]), strata, S=S)
    res = eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=1, strata=c.sp, cmh=True)
    cmh_p, r_cmh, p = res["cmh_p"].cpu().numpy(), res["r_cmh"].cpu().numpy(), res["p"].cpu().numpy()
    assert (cmh_p[0] == 1.0).all() and (r_cmh[0] == P).all() and np.isnan(res["cmh_stat"].cpu().numpy()[0]).all()
    assert p[0, 0] < 1e-6
    assert cmh_p[1, 5] < 1e-6 and cmh_p[1, 5] < min(cmh_p[1, 4], cmh_p[1, 6]) and r_cmh[1, 5] < P
    assert int(np.argmin(cmh_p[1])) == 5
