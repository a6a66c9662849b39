"""The rank-sum kernels (spec S15) on the GPU against the plain-Python restatement (ranksum_spec.py): k_ranksum's
observed statistic, k_ranksum_labels' permuted rows bit for bit, and k_permute_ranksum's exceedance counts, at the
shapes where they can go wrong -- a K tail and a gene-tile tail, heavy ties, several K chunks with a negative hi
digit, the largest matrix, a ragged last stage of permutations, two engine batches, traits of differing validity."""
import ctypes

import numpy as np
import pytest

import ranksum_spec as rs

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE1234567
ERR_SIZE = -3


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _values(name):
    """(genes [G, N] 0/1, values [T, N] with nan, P, budget_bytes of the B operand)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "tails":                      # K tail (257 = 8 words + 1 bit), gene-tile tail (300 = 256 + 44), T = 3
        G, N, P = 300, 257, 70
        vals = np.stack([np.round(rng.standard_normal(N), 1), rng.integers(0, 4, N).astype(float), np.full(N, 2.0)])
        vals[0, rng.random(N) < 0.2] = np.nan
        vals[1, rng.random(N) < 0.5] = np.nan
        vals[1, 256] = 1.0                   # the last isolate is valid
        budget = 3 * 2 * 32768               # three traits x two K chunks of 64 permutations: batches of 64 and 6
    elif name == "ties":
        G, N, P = 130, 129, 33
        vals = rng.integers(0, 6, (1, N)).astype(float)
        budget = 8 << 30
    elif name == "distinct":                 # nine K chunks, ranks past +-128 * 8: negative hi digits
        G, N, P = 70, 2100, 33
        vals = (rng.permutation(N) * 0.25 - 100.0)[None]
        budget = 8 << 30
    else:                                    # the largest matrix: 64 chunks, |Rc| up to 16 319
        assert name == "largest"
        G, N, P = 64, rs.MAX_ISOLATES, 3
        vals = (rng.permutation(N) * 1.0)[None]
        budget = 8 << 30
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[1] = 0
    genes[2] = 1
    genes[3] = 0
    genes[3, N - 1] = 1
    return genes, vals, P, budget


_CACHE = {}


def _case(eng, name):
    """Everything one shape needs, computed once: the device results and the restatement's."""
    if name in _CACHE:
        return _CACHE[name]
    genes, vals, P, budget = _values(name)
    T, N = vals.shape
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(vals)
    res = {k: v.cpu().numpy() for k, v in eng.ranksum(gm, plan).items()}
    rows = eng.ranksum_values(plan, 0, P, SEED).cpu().numpy()
    r = eng.ranksum_permute(gm, plan, eng.ranksum(gm, plan)["d"], P, SEED, budget_bytes=budget).cpu().numpy()
    spec = []
    for t in range(T):
        if N <= 3000:
            valid, rc, n, tiesum, _ = rs.ranks(vals[t].tolist())
        else:        # (the host ranking is held to the restatement in test_ranksum_spec.py; all distinct here)
            order = np.argsort(vals[t])
            rcv = np.empty(N, dtype=np.int64)
            rcv[order] = 2 * np.arange(N) + 2 - (N + 1)
            valid, rc, n, tiesum = [1] * N, rcv.tolist(), N, 0
        spec.append(dict(valid=valid, rc=rc, n=n, tiesum=tiesum,
                         rows=[rs.perm_row(SEED, t, pi, valid, rc) for pi in range(P)]))
    _CACHE[name] = dict(genes=genes, vals=vals, P=P, plan=plan, res=res, rows=rows, r=r, spec=spec, budget=budget)
    return _CACHE[name]


def _r_q(genes, rows, d_obs):
    """ranksum_spec.r_q in numpy (held to it on a few genes by the tests that use it)."""
    D = genes.astype(np.int64) @ np.asarray(rows, dtype=np.int64).T
    return (np.abs(D) >= np.abs(np.asarray(d_obs, dtype=np.int64))[:, None]).sum(axis=1)


CASES = ("tails", "ties", "distinct", "largest")


@pytest.mark.parametrize("name", CASES)
def test_observed_statistic(eng, name):
    c = _case(eng, name)
    genes, res = c["genes"], c["res"]
    untestable = 0
    for t, s in enumerate(c["spec"]):
        assert np.array_equal(c["plan"].rc_host[t], np.asarray(s["rc"])) and c["plan"].n[t] == s["n"]
        D = genes.astype(np.int64) @ np.asarray(s["rc"], dtype=np.int64)
        m = genes.astype(np.int64) @ np.asarray(s["valid"], dtype=np.int64)
        for g in (0, 3, len(genes) - 1):
            assert (int(D[g]), int(m[g])) == rs.statistic(genes[g].tolist(), s["valid"], s["rc"])
        assert np.array_equal(res["d"][t], D) and np.array_equal(res["m"][t], m)
        worst = 0.0
        for g in range(len(genes)):
            ok, auc, p = rs.tail(int(res["d"][t, g]), int(m[g]), s["n"], s["tiesum"])
            untestable += not ok
            assert res["auc"][t, g] == auc, (t, g)
            if not ok:
                assert res["p"][t, g] == 1.0 and res["d"][t, g] == 0
            else:
                # (no gene of these cases is a driver; where the restatement's p leaves the normal range or is
                # 0.0: test_gpu_ranksum_limits.py::test_p_of_a_driver_gene_down_to_the_underflow)
                assert p > 0
                worst = max(worst, abs(res["p"][t, g] - p) / p)
        print("%s trait %d: max relative p difference %.3g" % (name, t, worst))
        assert worst <= 1e-10
    assert untestable >= 2                      # the empty and the full gene at least


@pytest.mark.parametrize("name", CASES)
def test_permuted_rows_are_the_restatements_bit_for_bit(eng, name):
    c = _case(eng, name)
    assert c["rows"].dtype == np.int16
    for t, s in enumerate(c["spec"]):
        assert np.array_equal(c["rows"][t], np.asarray(s["rows"], dtype=np.int16)), (name, t)
    if name == "distinct":
        hi = [rs.digits(int(v))[0] for v in c["rows"][0, 0]]
        assert min(hi) < -8 and max(hi) > 8
    # a batch that starts later holds the same permutations
    later = eng.ranksum_values(c["plan"], c["P"] - 2, 2, SEED).cpu().numpy()
    assert np.array_equal(later, c["rows"][:, c["P"] - 2:])


@pytest.mark.parametrize("name", CASES)
def test_exceedance_counts_are_exact_twice_over(eng, name):
    c = _case(eng, name)
    genes, P = c["genes"], c["P"]
    for t, s in enumerate(c["spec"]):
        d_obs = c["res"]["d"][t]
        from_device_rows = _r_q(genes, c["rows"][t], d_obs)
        from_seed = _r_q(genes, s["rows"], d_obs)
        few = [0, 1, 2, 3, len(genes) - 1]
        assert rs.r_q([genes[g].tolist() for g in few], s["rows"], [int(d_obs[g]) for g in few]) == \
            from_seed[few].tolist()
        assert np.array_equal(c["r"][t], from_device_rows), (name, t)
        assert np.array_equal(c["r"][t], from_seed), (name, t)
        for g in range(len(genes)):
            if not rs.tail(int(d_obs[g]), int(c["res"]["m"][t, g]), s["n"], s["tiesum"])[0]:
                assert c["r"][t, g] == P
        assert c["r"][t, 1] == P and c["r"][t, 2] == P
    if name == "tails":
        assert (c["r"][2] == P).all()           # every value tied: no gene is testable
        assert eng.ranksum_batch(3, 257, P, c["budget"]) == 64 < P       # it ran as two batches
        assert c["r"][0].max() == P and ((0 < c["r"][0]) & (c["r"][0] < P)).any()


def test_one_batch_and_two_give_the_same_counts(eng):
    c = _case(eng, "tails")
    gm = eng.pack_dense(c["genes"])
    import torch
    d = torch.from_numpy(c["res"]["d"]).to(eng.device)
    assert eng.ranksum_batch(3, 257, c["P"]) == 128
    assert np.array_equal(eng.ranksum_permute(gm, c["plan"], d, c["P"], SEED).cpu().numpy(), c["r"])


def test_several_stages_of_permutations_per_block(eng):
    """Many gene blocks and sixteen stages of 64 permutations: with 512 blocks of 256 genes the launch gives a block
    more than one stage (a 256-CU device: eight ranges of two), so the accumulators start again and the counters
    carry on inside a block.  Few isolates keep the restatement quick: rows from the seed, counts by an exact
    float32 product (every sum is an integer below 2^24)."""
    rng = np.random.default_rng(77)
    G, N, P = 512 * 256, 33, 1000
    genes = (rng.random((G, N)) < 0.5).astype(np.uint8)
    vals = rng.integers(0, 9, (1, N)).astype(float)
    vals[0, 4] = np.nan
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(vals)
    d = eng.ranksum(gm, plan)["d"]
    r = eng.ranksum_permute(gm, plan, d, P, SEED).cpu().numpy()[0]
    valid, rc, n, tiesum, _ = rs.ranks(vals[0].tolist())
    rows = np.asarray([rs.perm_row(SEED, 0, pi, valid, rc) for pi in range(P)], dtype=np.float32)
    d_obs = genes.astype(np.float32) @ np.asarray(rc, dtype=np.float32)
    assert np.array_equal(d.cpu().numpy()[0], d_obs.astype(np.int32))
    want = np.empty(G, dtype=np.int64)
    for g0 in range(0, G, 16384):
        D = genes[g0:g0 + 16384].astype(np.float32) @ rows.T
        want[g0:g0 + 16384] = (np.abs(D) >= np.abs(d_obs[g0:g0 + 16384])[:, None]).sum(axis=1)
    few = [0, 255, 256, 70000, G - 1]
    assert rs.r_q([genes[g].tolist() for g in few], rows.astype(int).tolist(), [int(d_obs[g]) for g in few]) == \
        want[few].tolist()
    assert np.array_equal(r, want)
    assert want.max() <= P and (want < P).any() and (want > 0).any()


def test_too_many_isolates_are_refused_with_nothing_written(eng):
    import torch
    N, G, P = rs.MAX_ISOLATES + 1, 8, 2
    assert eng.ranksum_max_isolates() == rs.MAX_ISOLATES
    assert eng.lib.scoary_ranksum_bfrag_bytes(N, P, 1) == 0 < eng.lib.scoary_ranksum_bfrag_bytes(N - 1, P, 1)
    with pytest.raises(ValueError, match="at most 16320"):
        eng.ranksum_plan(np.zeros((1, N)))
    gm = eng.pack_dense(np.ones((G, N), dtype=np.uint8))
    dev = eng.device
    rc = torch.zeros((1, N), dtype=torch.int16, device=dev)
    valid = torch.zeros((1, eng.row_words(N)), dtype=torch.int32, device=dev)
    tiesum = torch.zeros((1,), dtype=torch.int64, device=dev)
    ints = [torch.full((1, G), 7, dtype=torch.int32, device=dev) for _ in range(3)]
    dbl = [torch.full((1, G), 7.0, dtype=torch.float64, device=dev) for _ in range(2)]
    rows = torch.full((1, P, N), 7, dtype=torch.int16, device=dev)
    bfrag = torch.full((1 << 16,), 7, dtype=torch.uint8, device=dev)
    p, s = eng._ptr, eng._stream()
    seed = ctypes.c_uint64(SEED)
    assert eng.lib.scoary_ranksum(eng.h, p(gm.tiled), p(rc), p(valid), p(tiesum), G, 1, N, p(ints[0]), p(ints[1]),
                                  p(dbl[0]), p(dbl[1]), s) == ERR_SIZE
    assert eng.lib.scoary_ranksum_perm_generate(eng.h, p(rc), p(valid), 1, N, P, 0, 0, seed, p(rows), s) == ERR_SIZE
    assert eng.lib.scoary_ranksum_perm_generate_bfrag(eng.h, p(rc), p(valid), 1, N, P, 0, 0, seed, p(bfrag),
                                                      s) == ERR_SIZE
    assert eng.lib.scoary_permute_ranksum(eng.h, p(gm.tiled), p(bfrag), p(ints[0]), G, 1, N, P, p(ints[2]),
                                          s) == ERR_SIZE
    assert b"scoary_ranksum_max_isolates" in eng.lib.scoary_last_error(eng.h)
    torch.cuda.synchronize()
    for x in ints + dbl + [rows, bfrag]:
        assert bool((x == 7).all())
    assert eng.lib.scoary_ranksum(eng.h, None, p(rc), p(valid), p(tiesum), G, 1, 10, p(ints[0]), p(ints[1]),
                                  p(dbl[0]), p(dbl[1]), s) == -1
    assert eng.lib.scoary_permute_ranksum(eng.h, p(gm.tiled), p(bfrag), p(ints[0]), G, 1, 10, -1, p(ints[2]), s) == -1
