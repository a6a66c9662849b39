"""The van Elteren kernels (spec S16) on the GPU, through the raw entry points and the engine, against the plain
Python restatement vanelteren_spec.py: the stratified generator's rows and B operand bit for bit, the stratum bits
up to 1024 strata, the size limit N = 16 320, one stratum against the S15 kernels, the observed statistic, and the
exceedance counts over batches.  test_gpu_vanelteren_limits.py holds the same kernels at their size edges, at every
width of the stratum field, at the ends of the counter words, over a full segment table and in the deep tail of p."""
import ctypes
import math

import numpy as np
import pytest

import ranksum_spec as rs
import vanelteren_spec as ve

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE1234567
ROW_FILL = 0x5A5A                   # no score: |a| <= 16 319


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _gen_rows(eng, plan, P, perm_base=0, seed=SEED):
    """scoary_vanelteren_perm_generate into a buffer filled with ROW_FILL -> int16 [T, P, N] on the host."""
    import torch
    out = torch.full((plan.T, P, plan.N), ROW_FILL, dtype=torch.int16, device=eng.device)
    eng._check(eng.lib.scoary_vanelteren_perm_generate(
        eng.h, eng._ptr(plan.l), eng._ptr(plan.valid), eng._ptr(plan.strata), plan.T, plan.N, plan.S, P, perm_base, 0,
        ctypes.c_uint64(seed), eng._ptr(out), eng._stream()), "scoary_vanelteren_perm_generate")
    return out.cpu().numpy()


def _gen_bfrag(eng, plan, P, perm_base=0):
    """scoary_vanelteren_perm_generate_bfrag into a buffer filled with 0xA5 -> its bytes on the host."""
    import torch
    nbytes = int(eng.lib.scoary_ranksum_bfrag_bytes(plan.N, P, plan.T))
    assert nbytes == rs.bfrag_bytes(plan.N, P, plan.T)
    buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=eng.device)
    eng._check(eng.lib.scoary_vanelteren_perm_generate_bfrag(
        eng.h, eng._ptr(plan.l), eng._ptr(plan.valid), eng._ptr(plan.strata), plan.T, plan.N, plan.S, P, perm_base, 0,
        ctypes.c_uint64(SEED), eng._ptr(buf), eng._stream()), "scoary_vanelteren_perm_generate_bfrag")
    return buf.cpu().numpy()


def _spec_plans(vals, st, S):
    return [ve.plan([float(v) for v in vals[t]], [int(s) for s in st], S) for t in range(vals.shape[0])]


def _spec_rows(pls, perms, seed=SEED):
    return np.asarray([[ve.perm_row(seed, t, pi, pl) for pi in perms] for t, pl in enumerate(pls)], dtype=np.int64)


def _counts(genes, rows, thr):
    """#{rows : |D| >= |thr|} per gene, D by a float64 product: every sum is an integer below 2^53, so exact."""
    D = genes.astype(np.float64) @ np.asarray(rows, dtype=np.float64).T
    return (np.abs(D) >= np.abs(np.asarray(thr, dtype=np.float64))[:, None]).sum(axis=1)


# ---------------------------------------------------------------- 1. rows and B operand bit for bit ------
def test_rows_and_b_operand_bit_for_bit(eng):
    """N = 77, S = 3 interleaved, T = 2 with different missing patterns (trait 1: stratum 1 without a valid isolate,
    stratum 2 with exactly one); P = 70 in one call and as perm_base 0 .. 40, 40 .. 70; the B operand is
    bfrag_encode of those rows, its zero K pad and its columns >= P included."""
    rng = np.random.default_rng(77)
    N, S, T, P = 77, 3, 2, 70
    st = np.arange(N) % 3
    vals = np.round(rng.standard_normal((T, N)), 1)
    vals[0, [4, 9, 50]] = np.nan
    vals[1, st == 1] = np.nan
    vals[1, st == 2] = np.nan
    vals[1, 5] = 0.3                                        # 5 mod 3 = 2: the one value of stratum 2
    plan = eng.vanelteren_plan(vals, st)
    assert plan.S == 3 and list(plan.n[1]) == [26, 0, 1]
    pls = _spec_plans(vals, st, S)
    want = _spec_rows(pls, range(P))
    assert np.array_equal(plan.score_host, [pl["score"] for pl in pls])
    assert np.array_equal(_gen_rows(eng, plan, P), want)
    assert np.array_equal(_gen_rows(eng, plan, 40), want[:, :40])
    assert np.array_equal(_gen_rows(eng, plan, 30, perm_base=40), want[:, 40:])
    assert np.array_equal(eng.vanelteren_values(plan, 40, 30, SEED).cpu().numpy(), want[:, 40:])
    for base, count in ((0, 70), (0, 40), (40, 30)):
        buf = _gen_bfrag(eng, plan, count, perm_base=base)
        assert np.array_equal(buf, rs.bfrag_encode(want[:, base:base + count], N)), (base, count)


# ---------------------------------------------------------------- 2. the stratum bits ------
@pytest.mark.parametrize("S", (1024, 1000))
def test_stratum_bits(eng, S):
    """N = 2100 over S = 1024 (b = 10) and S = 1000 (no power of two) strata drawn at random, so that some strata
    are empty, the last one in use; P = 5 rows are the restatement's."""
    rng = np.random.default_rng(S)
    N, P = 2100, 5
    st = rng.integers(0, S, N)
    st[7] = S - 1
    assert len(set(st.tolist())) < S                        # empty strata
    vals = np.round(rng.standard_normal((2, N)), 2)
    vals[1, rng.random(N) < 0.3] = np.nan
    plan = eng.vanelteren_plan(vals, st)
    assert plan.S == S and ve.strata_bits(S) == 10
    want = _spec_rows(_spec_plans(vals, st, S), range(P))
    assert np.array_equal(_gen_rows(eng, plan, P), want)
    got = rs.bfrag_decode(_gen_bfrag(eng, plan, P), 2, P, N)[0]
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 3. the size limit ------
@pytest.mark.parametrize("sizes", ((16319, 1), (8160, 8160)))
def test_size_limit(eng, sizes):
    """N = 16 320 = scoary_ranksum_max_isolates() in strata of (16 319, 1) and (8 160, 8 160): w = 1, |a| up to
    16 318.  P = 3 rows, and D, m and r of G = 300 genes, are the restatement's."""
    rng = np.random.default_rng(sizes[0])
    N, P, G = 16320, 3, 300
    assert N == eng.ranksum_max_isolates()
    st = rng.permutation(np.repeat([0, 1], sizes))
    vals = rng.standard_normal((1, N))                      # no ties: the extreme scores occur
    plan = eng.vanelteren_plan(vals, st)
    pls = _spec_plans(vals, st, 2)
    assert pls[0]["w"] == [1, ve.weight(sizes[1])] and max(np.abs(pls[0]["score"])) >= sizes[0] - 1
    want = _spec_rows(pls, range(P))[0]
    assert np.array_equal(_gen_rows(eng, plan, P)[0], want)
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[0], genes[1] = 0, 1
    genes[2] = st == 1
    gm = eng.pack_dense(genes)
    res = eng.vanelteren(gm, plan)
    d = genes.astype(np.int64) @ np.asarray(pls[0]["score"], dtype=np.int64)
    assert np.array_equal(res["d"].cpu().numpy()[0], d)
    assert np.array_equal(res["m"].cpu().numpy()[0], genes.sum(axis=1))
    assert d[0] == 0 and d[1] == 0 and d[2] == 0 and res["p"].cpu().numpy()[0, :3].tolist() == [1.0, 1.0, 1.0]
    r = eng.vanelteren_permute(gm, plan, res["d"], P, SEED).cpu().numpy()[0]
    assert np.array_equal(r, _counts(genes, want, d))
    assert r[:3].tolist() == [P, P, P]


# ---------------------------------------------------------------- 4. one stratum ------
def test_one_stratum_is_the_rank_sum_generator(eng):
    """S = 1: the rows are w_0 x the rows of scoary_ranksum_perm_generate at the same seed, r is ranksum_permute's."""
    rng = np.random.default_rng(41)
    N, T, P, G = 300, 2, 100, 200
    vals = np.round(rng.standard_normal((T, N)), 1)
    vals[1, ::9] = np.nan
    plan = eng.vanelteren_plan(vals, np.zeros(N, dtype=np.int64))
    rplan = eng.ranksum_plan(vals)
    w0 = plan.w[:, 0]
    assert plan.S == 1 and list(w0) == [16319 // (int(n) + 1) for n in rplan.n]
    rows = _gen_rows(eng, plan, P, seed=9)
    base = eng.ranksum_values(rplan, 0, P, 9).cpu().numpy().astype(np.int64)
    assert np.array_equal(rows, base * w0[:, None, None])
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    gm = eng.pack_dense(genes)
    res, rres = eng.vanelteren(gm, plan), eng.ranksum(gm, rplan)
    assert np.array_equal(res["d"].cpu().numpy(), rres["d"].cpu().numpy() * w0[:, None])
    assert np.array_equal(res["m"].cpu().numpy(), rres["m"].cpu().numpy())
    r = eng.vanelteren_permute(gm, plan, res["d"], P, 9).cpu().numpy()
    assert np.array_equal(r, eng.ranksum_permute(gm, rplan, rres["d"], P, 9).cpu().numpy())
    assert 0 < r.sum() < T * G * P


# ---------------------------------------------------------------- 5. / 6. the observed statistic, r ------
@pytest.fixture(scope="module")
def case5(eng):
    """N = 333 (no multiple of 32 or 128), G = 600 (three blocks, the last one partial), S = 9 interleaved, T = 3."""
    rng = np.random.default_rng(555)
    N, G, S, T = 333, 600, 9, 3
    st = np.arange(N) % S
    vals = np.round(rng.standard_normal((T, N)), 1)
    vals[1, rng.random(N) < 0.25] = np.nan
    vals[2, st == 4] = 2.0                                  # a fully tied stratum
    vals[2, st == 6] = np.nan                               # ... and one without a value
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[0] = 0
    genes[1] = 1
    genes[2] = 0
    genes[2, (st == 3) & (rng.random(N) < 0.5)] = 1         # confined to one stratum
    genes[3] = np.isin(st, (0, 5, 8))                       # whole strata only: untestable
    genes[599] = genes[2]
    plan = eng.vanelteren_plan(vals, st)
    return dict(N=N, G=G, S=S, T=T, st=st, vals=vals, genes=genes, plan=plan, gm=eng.pack_dense(genes),
                pls=_spec_plans(vals, st, S))


def test_observed_statistic(eng, case5):
    c = case5
    res = {k: v.cpu().numpy() for k, v in eng.vanelteren(c["gm"], c["plan"]).items()}
    worst_p = worst_var = 0.0
    ntest = 0
    for t, pl in enumerate(c["pls"]):
        for g, gene in enumerate(c["genes"]):
            D, ms = ve.statistic(gene, pl)
            ok, var, den, auc, p = ve.tail(D, ms, pl)
            assert (res["d"][t, g], res["m"][t, g]) == (D, sum(ms)), (t, g)
            assert (res["var"][t, g] > 0) == ok, (t, g)
            assert res["auc"][t, g] == auc, (t, g)                       # bit-equal: den is exact
            if not ok:
                assert D == 0 and res["p"][t, g] == 1.0 and res["var"][t, g] == 0.0
                continue
            ntest += 1
            worst_var = max(worst_var, abs(res["var"][t, g] - var) / var)
            z = (abs(int(res["d"][t, g])) * 0.5) / math.sqrt(res["var"][t, g])
            ref = math.erfc(z / math.sqrt(2.0))
            worst_p = max(worst_p, abs(res["p"][t, g] - ref) / ref)
    print("van Elteren observed statistic: %d testable cells, worst relative error of var %.3g, of p %.3g"
          % (ntest, worst_var, worst_p))
    assert not res["var"][:, :2].any() and not res["var"][:, 3].any() and res["var"][:2, 2].all()
    assert 0.9 * c["T"] * c["G"] < ntest < c["T"] * c["G"]
    assert worst_var == 0.0                                 # the order is fixed and contraction is off
    assert worst_p < 1e-10


def test_r_through_the_engine_in_batches(eng, case5):
    """P = 130 under a budget that forces batches of 64: r from the seed alone equals r counted over rows read
    back, and the restatement's r on the restatement's rows."""
    c = case5
    plan, P = c["plan"], 130
    d = eng.vanelteren(c["gm"], plan)["d"]
    budget = int(eng.lib.scoary_ranksum_bfrag_bytes(c["N"], 64, c["T"]))
    assert eng.ranksum_batch(c["T"], c["N"], P, budget) == 64
    r = eng.vanelteren_permute(c["gm"], plan, d, P, SEED, budget_bytes=budget).cpu().numpy()
    rows = eng.vanelteren_values(plan, 0, P, SEED).cpu().numpy()
    want = _spec_rows(c["pls"], range(P))
    assert np.array_equal(rows, want)
    for t, pl in enumerate(c["pls"]):
        d_spec = c["genes"].astype(np.int64) @ np.asarray(pl["score"], dtype=np.int64)
        assert np.array_equal(r[t], _counts(c["genes"], rows[t], d_spec)), t
    sample = list(range(0, c["G"], 40)) + [1, 2, 3, 599]
    for t, pl in enumerate(c["pls"]):
        d_obs = [ve.statistic(c["genes"][g], pl)[0] for g in sample]
        assert list(r[t, sample]) == ve.r_counts([c["genes"][g] for g in sample], want[t].tolist(), d_obs), t
    assert (r[:, [0, 1, 3]] == P).all() and 0 < r.sum() < c["T"] * c["G"] * P
