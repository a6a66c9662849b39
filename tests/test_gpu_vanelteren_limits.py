"""The van Elteren kernels (spec S16) at their limits, against the restatement vanelteren_spec.py.

a. k_vanelteren_labels at its size edges, rows bit for bit and the whole B operand byte for byte
   (ranksum_spec.bfrag_encode, K pad and the columns from P on included): N and the number n of valid isolates at
   the edges of a word, of a chunk of 256, of the 2048-byte floor under the keys, of a sort size (n = 2^k against
   2^k + 1), of a lane's second held entry (n > 1024) and of the 64 KB of dynamic LDS (N = 4096 against 4097); traits
   of 0, 1 and 2 valid isolates.
b. The stratum field of the composite at every width from one bit to four (S = 2, 3, 4, 5, 8, 9).
c. The counter words: trait_base and perm_base as part of the counter, up to 2^32 exactly, refused one past it.
d. k_vanelteren where the segment table is fullest -- N = 16 320 segments of one isolate each, strata that restart at
   word 0 (the quad reload goes backwards), the same strata contiguous, 1024 strata drawn at random -- and G at
   255 / 256 / 257: d, m, var and auc bit-equal, p within 1e-10 relative of erfc at the device's own z.
e. p into the deep tail, down to the underflow of erfc, under test_gpu_ranksum_limits' rule.

(test_gpu_vanelteren.py holds the same kernels at moderate shapes and end to end.)"""
import ctypes
import math

import numpy as np
import pytest

import ranksum_spec as rs
import vanelteren_spec as ve
from test_gpu_vanelteren import ROW_FILL, SEED, _spec_plans

pytestmark = pytest.mark.gpu
ERR_SIZE = -3                       # SCOARY_ERR_SIZE of include/scoary_hip.h
DBL_MIN = 2.2250738585072014e-308
MAX_N = 16320


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- the raw entry points ------
def _generate(eng, plan, P, perm_base=0, trait_base=0, bfrag=False):
    """scoary_vanelteren_perm_generate into int16 [T, P, N] of ROW_FILL, or ..._bfrag into bytes of 0xA5 ->
    (return code, the buffer on the host)."""
    import torch
    if bfrag:
        nbytes = int(eng.lib.scoary_ranksum_bfrag_bytes(plan.N, P, plan.T))
        assert nbytes == rs.bfrag_bytes(plan.N, P, plan.T)
        out = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=eng.device)
        call = eng.lib.scoary_vanelteren_perm_generate_bfrag
    else:
        out = torch.full((plan.T, P, plan.N), ROW_FILL, dtype=torch.int16, device=eng.device)
        call = eng.lib.scoary_vanelteren_perm_generate
    rc = call(eng.h, eng._ptr(plan.l), eng._ptr(plan.valid), eng._ptr(plan.strata), plan.T, plan.N, plan.S, P,
              perm_base, trait_base, ctypes.c_uint64(SEED), eng._ptr(out), eng._stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _rows(eng, plan, P, **kw):
    rc, out = _generate(eng, plan, P, **kw)
    eng._check(rc, "scoary_vanelteren_perm_generate")
    return out


def _bfrag(eng, plan, P, **kw):
    rc, out = _generate(eng, plan, P, bfrag=True, **kw)
    eng._check(rc, "scoary_vanelteren_perm_generate_bfrag")
    return out


def _want(pls, P, perm_base=0, trait_base=0):
    """The restatement's rows [T, P, N] at the counters trait_base + t, perm_base + p."""
    return np.asarray([[ve.perm_row(SEED, trait_base + t, perm_base + p, pl) for p in range(P)]
                       for t, pl in enumerate(pls)], dtype=np.int64)


def _observed(eng, gm, plan):
    """scoary_vanelteren into prefilled outputs -> dict of host arrays [T, G]."""
    import torch
    T, G = plan.T, gm.G
    out = {k: torch.full((T, G), -777, dtype=torch.int32, device=eng.device) for k in ("d", "m")}
    out.update({k: torch.full((T, G), math.nan, dtype=torch.float64, device=eng.device) for k in ("var", "auc", "p")})
    eng._check(eng.lib.scoary_vanelteren(
        eng.h, eng._ptr(gm.tiled), eng._ptr(plan.score), eng._ptr(plan.valid), eng._ptr(plan.strata),
        eng._ptr(plan.members), eng._ptr(plan.wn), eng._ptr(plan.c), G, T, plan.N, plan.S,
        *(eng._ptr(out[k]) for k in ("d", "m", "var", "auc", "p")), eng._ptr(eng._cmh_scratch(plan.N)), eng._stream()),
        "scoary_vanelteren")
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---------------------------------------------------------------- a. generator sizes ------
# N -> the valid isolates of trait 1 (trait 0 has all N): a power of two at one N, one above it at the next
_N1 = {1: 0, 2: 1, 31: 16, 32: 17, 33: 32, 255: 128, 256: 129, 257: 256, 1024: 512, 1025: 1024, 1026: 1025,
       2049: 2048, 4096: 2049, 4097: 4096, 8192: 4097, 8193: 8192}


@pytest.mark.parametrize("N", tuple(_N1))
def test_generator_sizes(eng, N):
    """T = 2, S = 3 interleaved (fewer where N < 3); P = 66 up to N = 257 -- a second stage, and 62 columns of it
    written by blocks of their own -- and P = 2 above (the restatement's Philox is the cost)."""
    rng = np.random.default_rng(N)
    T, P = 2, 66 if N <= 257 else 2
    st = np.arange(N) % 3
    vals = np.round(rng.standard_normal((T, N)), 1)
    vals[1, rng.permutation(N)[:N - _N1[N]]] = np.nan
    plan = eng.vanelteren_plan(vals, st)
    assert plan.S == min(N, 3) and plan.n.sum(axis=1).tolist() == [N, _N1[N]]
    pls = _spec_plans(vals, st, plan.S)
    want = _want(pls, P)
    assert np.array_equal(plan.score_host, [pl["score"] for pl in pls])
    assert np.array_equal(_rows(eng, plan, P), want)
    buf = _bfrag(eng, plan, P)
    assert np.array_equal(buf, rs.bfrag_encode(want, N))
    assert buf.size == T * -(-P // 64) * -(-N // 256) * 32768
    if _N1[N] == 0:
        assert not want[1].any()


def test_traits_of_zero_one_and_two_valid_isolates(eng):
    """N = 77, S = 3 interleaved, P = 66: a trait without a value (rows of zeros), one with one value (its score is
    0), one with two values in one stratum (scores +-w, both orders occur) and in two strata, and a full trait."""
    rng = np.random.default_rng(77)
    N, P = 77, 66
    st = np.arange(N) % 3
    vals = np.full((5, N), np.nan)
    vals[1, N - 1] = 2.5
    vals[2, [4, 76]] = [1.0, -1.0]                          # 4 and 76 are 1 mod 3
    vals[3, [0, 76]] = [1.0, -1.0]                          # strata 0 and 1: one value each
    vals[4] = np.round(rng.standard_normal(N), 1)
    plan = eng.vanelteren_plan(vals, st)
    assert plan.n.sum(axis=1).tolist() == [0, 1, 2, 2, N]
    pls = _spec_plans(vals, st, 3)
    want = _want(pls, P)
    got = _rows(eng, plan, P)
    assert np.array_equal(got, want)
    assert not got[0].any() and not got[1].any() and not got[3].any()
    w = ve.weight(2)
    assert {tuple(r) for r in got[2][:, [4, 76]].tolist()} == {(w, -w), (-w, w)} and np.abs(got[2]).sum() == 2 * w * P
    assert np.array_equal(_bfrag(eng, plan, P), rs.bfrag_encode(want, N))


# ---------------------------------------------------------------- b. stratum bits ------
@pytest.mark.parametrize("S", (2, 3, 4, 5, 8, 9))
def test_stratum_field_widths(eng, S):
    """N = 100, P = 5, strata drawn at random with the last one in use and, from S = 4 on, one without a member."""
    rng = np.random.default_rng(S)
    N, P = 100, 5
    st = rng.integers(0, S, N)
    empty = S // 2 if S >= 4 else None
    if empty is not None:
        st[st == empty] = 0
    st[7] = S - 1
    assert set(st.tolist()) == set(range(S)) - {empty}
    vals = np.round(rng.standard_normal((2, N)), 1)
    vals[1, rng.random(N) < 0.3] = np.nan
    plan = eng.vanelteren_plan(vals, st)
    assert plan.S == S and ve.strata_bits(S) == {2: 1, 3: 2, 4: 2, 5: 3, 8: 3, 9: 4}[S]
    want = _want(_spec_plans(vals, st, S), P)
    assert np.array_equal(_rows(eng, plan, P), want)
    got, _dig, pad, rest = rs.bfrag_decode(_bfrag(eng, plan, P), 2, P, N)
    assert np.array_equal(got, want) and not pad.any() and not rest.any()


# ---------------------------------------------------------------- c. counter words ------
def _counter_case(eng, T):
    """T traits of N = 100 over S = 3 with the same values in every trait."""
    rng = np.random.default_rng(100)
    N = 100
    st = rng.integers(0, 3, N)
    row = np.round(rng.standard_normal(N), 1)
    row[rng.random(N) < 0.2] = np.nan
    vals = np.tile(row, (T, 1))
    return eng.vanelteren_plan(vals, st), _spec_plans(vals, st, 3)


def test_trait_base_and_perm_base_are_part_of_the_counter(eng):
    big, pls = _counter_case(eng, 4)
    one, _ = _counter_case(eng, 1)
    all4 = _rows(eng, big, 9)
    got = _rows(eng, one, 4, perm_base=5, trait_base=3)
    assert np.array_equal(got[0], all4[3, 5:9])
    assert np.array_equal(all4, _want(pls, 9)) and np.array_equal(got, _want(pls[:1], 4, perm_base=5, trait_base=3))
    assert not np.array_equal(got[0], all4[3, :4]) and not np.array_equal(got[0], all4[0, 5:9])
    b4 = rs.bfrag_decode(_bfrag(eng, big, 9), 4, 9, big.N)[0]
    b1 = rs.bfrag_decode(_bfrag(eng, one, 4, perm_base=5, trait_base=3), 1, 4, one.N)[0]
    assert np.array_equal(b4, all4) and np.array_equal(b1, got)


def test_counter_words_up_to_two_to_the_32(eng):
    """perm_base + P = 2^32 and trait_base + T = 2^32 are taken, and are the restatement's at those counters; one more
    of either is SCOARY_ERR_SIZE, and the buffer keeps its fill."""
    plan, pls = _counter_case(eng, 2)
    P = 3
    for kw in (dict(perm_base=2 ** 32 - P), dict(trait_base=2 ** 32 - 2), dict(perm_base=2 ** 32 - P, trait_base=2 ** 32 - 2)):
        want = _want(pls, P, **kw)
        assert np.array_equal(_rows(eng, plan, P, **kw), want), kw
        assert np.array_equal(_bfrag(eng, plan, P, **kw), rs.bfrag_encode(want, plan.N)), kw
    assert not np.array_equal(_want(pls, P, perm_base=2 ** 32 - P), _want(pls, P, trait_base=2 ** 32 - 2))
    for kw in (dict(perm_base=2 ** 32 - P + 1), dict(trait_base=2 ** 32 - 1)):
        rc, rows = _generate(eng, plan, P, **kw)
        assert rc == ERR_SIZE and (rows == ROW_FILL).all(), kw
        rc, buf = _generate(eng, plan, P, bfrag=True, **kw)
        assert rc == ERR_SIZE and (buf == 0xA5).all(), kw


# ---------------------------------------------------------------- d. the observed statistic ------
def _plan(values, st, S):
    """ve.plan with a stratum's members looked up, not searched for among all isolates (ve.plan is O(S N): minutes at
    N = 16 320 and S = 1024); the same statements otherwise, and held to ve.plan at N = 333."""
    N = len(values)
    valid = [0 if math.isnan(x) else 1 for x in values]
    order = np.argsort(st, kind="stable")
    bounds = np.searchsorted(np.asarray(st)[order], np.arange(S + 1))
    score, L, w, n, tiesum, c = [0] * N, [], [], [], [], []
    for s in range(S):
        who = [int(i) for i in order[bounds[s]:bounds[s + 1]] if valid[i]]
        _valid, rc, ns, ts, _groups = rs.ranks([values[i] for i in who])
        ws = ve.weight(ns)
        for i, r in zip(who, rc):
            score[i] = ws * r
            L.append(ws * r)
        f = float(ns + 1) - float(ts) / (float(ns) * float(ns - 1)) if ns >= 2 else 0.0
        w.append(ws), n.append(ns), tiesum.append(ts), c.append(float(ws * ws) * f / 12.0)
    return dict(valid=valid, score=score, L=L, w=w, n=n, tiesum=tiesum, c=c, strata=[int(s) for s in st], S=S)


def _hold_observed(res, genes, st, pls, sample, label):
    """Every (trait, gene) of ``res`` against the restatement: D and the m_s of all genes by numpy, held to
    ve.statistic at the genes of ``sample`` (all genes where it is None), var / den / auc / p by ve.tail."""
    T, G = len(pls), len(genes)
    assert all(res[k].shape == (T, G) for k in ("d", "m", "var", "auc", "p"))
    worst_p, ntest = 0.0, 0
    for t, pl in enumerate(pls):
        valid = np.asarray(pl["valid"], dtype=bool)
        D = genes.astype(np.int64) @ np.asarray(pl["score"], dtype=np.int64)
        for g in range(G):
            ms = np.bincount(st[(genes[g] != 0) & valid], minlength=pl["S"]).tolist()
            if sample is None or g in sample:
                assert ve.statistic(genes[g].tolist(), pl) == (int(D[g]), ms), (t, g)
            ok, var, _den, auc, _p = ve.tail(int(D[g]), ms, pl)
            assert (res["d"][t, g], res["m"][t, g]) == (D[g], sum(ms)), (t, g)
            assert res["var"][t, g] == var and res["auc"][t, g] == auc, (t, g)       # bit-equal: the order is fixed
            if not ok:
                assert D[g] == 0 and var == 0.0 and res["p"][t, g] == 1.0, (t, g)
                continue
            ntest += 1
            z = (abs(int(res["d"][t, g])) * 0.5) / math.sqrt(res["var"][t, g])
            ref = math.erfc(z / math.sqrt(2.0))
            assert ref > 0.0
            worst_p = max(worst_p, abs(res["p"][t, g] - ref) / ref)
    print("van Elteren observed statistic, %s: %d of %d cells testable, var and auc bit-equal, worst relative error "
          "of p %.3g" % (label, ntest, T * G, worst_p))
    assert worst_p < 1e-10
    return ntest


def _layout(name):
    rng = np.random.default_rng(1024)
    if name == "interleaved":                   # stratum s = isolates s, s + 1024, ...: a word each, from word s / 32 on
        return np.arange(MAX_N) % 1024
    if name == "contiguous":                    # the same strata, each in one or two words
        return np.sort(np.arange(MAX_N) % 1024)
    st = rng.integers(0, 1024, MAX_N)
    st[st % 97 == 5] = 1023                     # strata without a member; the last one in use
    return st


@pytest.mark.parametrize("name", ("interleaved", "contiguous", "random"))
def test_observed_statistic_over_1024_strata(eng, name):
    """N = 16 320 over 1024 strata, T = 2 (a quarter of trait 1 missing), G = 257 (a second block of one gene)."""
    N, T, G, S = MAX_N, 2, 257, 1024
    st = _layout(name)
    rng = np.random.default_rng(len(name))
    vals = np.round(rng.standard_normal((T, N)), 1)
    vals[1, rng.random(N) < 0.25] = np.nan
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[0] = 0
    genes[1] = 1
    genes[2] = (st == st[0]) & (rng.random(N) < 0.5)        # confined to one stratum
    genes[2, 0] = 1
    genes[3] = np.isin(st, rng.permutation(S)[:300])        # whole strata only: untestable
    genes[4] = 0
    genes[4, N - 1] = 1                                     # the last isolate only
    genes[5] = st & 1                                       # "the stratum is odd": whole strata again
    genes[256] = genes[2]
    plan = eng.vanelteren_plan(vals, st)
    members = len(set(st.tolist()))
    if name == "interleaved":                               # one isolate per (stratum, word): N segments, the table's limit
        assert len(set(zip(st.tolist(), (np.arange(N) // 32).tolist()))) == N and members == S
    if name == "random":
        assert members < S and st.max() == S - 1
    pls = [_plan(vals[t].tolist(), st, S) for t in range(T)]
    assert np.array_equal(plan.score_host, [pl["score"] for pl in pls])
    assert np.array_equal(plan.n, [pl["n"] for pl in pls]) and np.array_equal(plan.w, [pl["w"] for pl in pls])
    res = _observed(eng, eng.pack_dense(genes), plan)
    sample = {0, 1, 2, 3, 4, 5, 255, 256} | set(range(6, G, 25))
    assert len(sample) >= 16
    ntest = _hold_observed(res, genes, st, pls, sample, "N %d, %s strata" % (N, name))
    assert not res["var"][:, [0, 1, 3, 5]].any() and res["var"][:, 2].all() and ntest > 0.9 * T * G
    assert np.array_equal(res["d"][:, 256], res["d"][:, 2]) and np.array_equal(res["p"][:, 256], res["p"][:, 2])


@pytest.mark.parametrize("G", (255, 256))
def test_observed_statistic_at_the_edge_of_a_block_of_genes(eng, G):
    """test_gpu_vanelteren's shape (N = 333, S = 9 interleaved, T = 3) at G = 255 and 256; every cell by ve.statistic."""
    rng = np.random.default_rng(G)
    N, S, T = 333, 9, 3
    st = np.arange(N) % S
    vals = np.round(rng.standard_normal((T, N)), 1)
    vals[1, rng.random(N) < 0.25] = np.nan
    vals[:2, N - 1] = 0.3                                   # (the last isolate has a value)
    vals[2, st == 4] = 2.0
    vals[2, st == 6] = np.nan
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[0] = 0
    genes[G - 2] = 1
    genes[G - 1] = 0
    genes[G - 1, N - 1] = 1
    pls = _spec_plans(vals, st, S)
    assert all(_plan(vals[t].tolist(), st, S) == pl for t, pl in enumerate(pls))       # (_plan is ve.plan)
    res = _observed(eng, eng.pack_dense(genes), eng.vanelteren_plan(vals, st))
    assert _hold_observed(res, genes, st, pls, None, "N %d, G %d" % (N, G)) > 0.9 * T * G
    assert not res["var"][:, [0, G - 2]].any() and res["var"][:2, G - 1].all()


# ---------------------------------------------------------------- e. the deep tail of p ------
def _driver_p(h):
    """The restatement's p of two strata of h distinct values each and the gene "above the stratum's median"."""
    w, m = ve.weight(h), h // 2
    c = float(w * w) * float(h + 1) / 12.0
    pl = dict(S=2, c=[c, c], n=[h, h], w=[w, w])
    return ve.tail(2 * w * m * (h - m), [m, m], pl)[4]


def test_p_of_a_driver_gene_down_to_the_underflow(eng):
    """Two strata of 1050 isolates; a trait has h distinct values in each, and its gene is "the value lies above the
    median of its stratum's values": D = 2 w m (h - m), z grows like sqrt(1.5 h), and p leaves the normal range of
    doubles between h = 900 and h = 1050.  The rule is test_gpu_ranksum_limits': 1e-10 relative where the
    restatement's p is normal; below 2.2250738585072014e-308 each side rounds to the subnormal grid once, 1e-10
    relative plus two grid steps; where it is 0.0, 0.0."""
    H = 1050
    N = 2 * H
    sub = [h for h in range(900, H + 1) if 0.0 < _driver_p(h) < DBL_MIN]
    assert sub and _driver_p(H) == 0.0 and _driver_p(900) >= DBL_MIN
    hs = [300, 500, 900, sub[0], sub[len(sub) // 2], H]
    st = np.repeat([0, 1], H)
    rng = np.random.default_rng(6)
    vals = np.full((len(hs), N), np.nan)
    genes = np.zeros((len(hs), N), dtype=np.uint8)
    for t, h in enumerate(hs):
        for s in (0, 1):
            idx = s * H + rng.permutation(H)[:h]
            vals[t, idx] = rng.permutation(h) * 0.5
            genes[t, idx] = vals[t, idx] > np.median(vals[t, idx])
    plan = eng.vanelteren_plan(vals, st)
    res = _observed(eng, eng.pack_dense(genes), plan)
    pls = _spec_plans(vals, st, 2)
    seen = set()
    for t, h in enumerate(hs):
        pl = pls[t]
        assert pl["n"] == [h, h] and pl["tiesum"] == [0, 0]
        for g in range(len(hs)):
            D, ms = ve.statistic(genes[g].tolist(), pl)
            ok, var, _den, auc, p = ve.tail(D, ms, pl)
            got = float(res["p"][t, g])
            assert ok and (res["d"][t, g], res["m"][t, g]) == (D, sum(ms))
            assert res["var"][t, g] == var and res["auc"][t, g] == auc
            kind = "zero" if p == 0.0 else "subnormal" if p < DBL_MIN else "normal"
            if g == t:
                m = h // 2
                assert ms == [m, m] and D == 2 * pl["w"][0] * m * (h - m) and auc == 1.0 and p == _driver_p(h)
                seen.add(kind)
                print("h = %d: p %.17g, restatement %.17g (%s), difference %.3g"
                      % (h, got, p, kind, abs(got - p) / p if p else abs(got - p)))
            if kind == "zero":
                assert got == 0.0, (h, g, got)
            elif kind == "subnormal":
                assert abs(got - p) <= 1e-10 * p + 2 * 4.94e-324, (h, g, got, p)
            else:
                assert abs(got - p) <= 1e-10 * p, (h, g, got, p)
    assert seen == {"normal", "subnormal", "zero"}
