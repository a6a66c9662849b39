"""The rank-sum kernels (spec S15) at their limits, through the raw entry points: what k_ranksum_labels writes as
the B operand, byte for byte against the layout include/scoary_hip.h states (ranksum_spec.bfrag_encode); the trait
base of the counter word; traits of 0, 1 and 2 valid isolates and isolate counts at the edges of a word, a chunk, a
sort size, a lane's second entry and the 64 KB of dynamic LDS, through all three kernels; k_permute_ranksum over a
B operand the test builds itself -- several stages per block with several K chunks, a ragged last range, |D| pinned
per cell up to the largest sum the contract allows, equality and sign of the threshold, a d_r that does not start
at zero -- and k_ranksum's p down to the underflow of erfc.  (test_gpu_ranksum.py holds the same kernels end to end
at moderate shapes.)"""
import ctypes
import math

import numpy as np
import pytest

import ranksum_spec as rs
from test_gpu_ranksum import _values

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE1234567
ROW_FILL = 0x5A5A                   # no centred rank: |Rc| <= 16 319
DBL_MIN = 2.2250738585072014e-308
R0 = 5                              # where d_r starts: batches add up


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
def _dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _gen_rows(eng, rc, valid, T, N, P, perm_base=0, trait_base=0):
    """scoary_ranksum_perm_generate into a buffer filled with ROW_FILL -> int16 [T, P, N] on the host."""
    import torch
    out = torch.full((T, P, N), ROW_FILL, dtype=torch.int16, device=eng.device)
    eng._check(eng.lib.scoary_ranksum_perm_generate(eng.h, eng._ptr(rc), eng._ptr(valid), T, N, P, perm_base,
                                                    trait_base, ctypes.c_uint64(SEED), eng._ptr(out), eng._stream()),
               "scoary_ranksum_perm_generate")
    return out.cpu().numpy()


def _gen_bfrag(eng, rc, valid, T, N, P, perm_base=0, trait_base=0):
    """scoary_ranksum_perm_generate_bfrag into a buffer filled with 0xA5 -> the device tensor of its bytes."""
    import torch
    nbytes = int(eng.lib.scoary_ranksum_bfrag_bytes(N, P, T))
    assert nbytes == rs.bfrag_bytes(N, P, T) == T * ((P + 63) // 64) * ((N + 255) // 256) * 32768
    buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=eng.device)
    eng._check(eng.lib.scoary_ranksum_perm_generate_bfrag(eng.h, eng._ptr(rc), eng._ptr(valid), T, N, P, perm_base,
                                                          trait_base, ctypes.c_uint64(SEED), eng._ptr(buf),
                                                          eng._stream()), "scoary_ranksum_perm_generate_bfrag")
    return buf


def _permute(eng, gm, bfrag, dobs, T, N, P, start=0):
    """scoary_permute_ranksum onto a d_r that holds `start` everywhere -> int32 [T, G] on the host."""
    import torch
    if isinstance(bfrag, np.ndarray):
        bfrag = _dev(eng, bfrag)
    dobs = _dev(eng, np.asarray(dobs, dtype=np.int32).reshape(T, gm.G))
    r = torch.full((T, gm.G), start, dtype=torch.int32, device=eng.device)
    eng._check(eng.lib.scoary_permute_ranksum(eng.h, eng._ptr(gm.tiled), eng._ptr(bfrag), eng._ptr(dobs), gm.G, T, N,
                                              P, eng._ptr(r), eng._stream()), "scoary_permute_ranksum")
    return r.cpu().numpy()


def _observed(eng, gm, plan):
    """scoary_ranksum into prefilled outputs -> dict of host arrays [T, G]."""
    import torch
    T, G = plan.T, gm.G
    out = {"d": torch.full((T, G), -777, dtype=torch.int32, device=eng.device),
           "m": torch.full((T, G), -777, dtype=torch.int32, device=eng.device),
           "auc": torch.full((T, G), math.nan, dtype=torch.float64, device=eng.device),
           "p": torch.full((T, G), math.nan, dtype=torch.float64, device=eng.device)}
    eng._check(eng.lib.scoary_ranksum(eng.h, eng._ptr(gm.tiled), eng._ptr(plan.rc), eng._ptr(plan.valid),
                                      eng._ptr(plan.tiesum), G, T, plan.N,
                                      *(eng._ptr(out[k]) for k in ("d", "m", "auc", "p")), eng._stream()),
               "scoary_ranksum")
    return {k: v.cpu().numpy() for k, v in out.items()}


def _genes(rng, G, N):
    """Random densities, plus the empty, the full and the last-isolate-only gene (test_gpu_ranksum._values')."""
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[1] = 0
    genes[2] = 1
    genes[3] = 0
    genes[3, N - 1] = 1
    return genes


def _counts(genes, rows, thr):
    """#{columns : |D| >= |thr|} per gene, D by a float64 product: every sum is an integer below 2^53, so exact."""
    D = genes.astype(np.float64) @ np.asarray(rows, dtype=np.float64).T
    assert np.abs(D).max(initial=0) < 2.0 ** 53
    return (np.abs(D) >= np.abs(np.asarray(thr, dtype=np.float64))[:, None]).sum(axis=1), D


def _spec_rows(t, perms, valid, rc):
    return np.asarray([rs.perm_row(SEED, t, pi, valid, rc) for pi in perms], dtype=np.int64)


# ---------------------------------------------------------------- a. the generator's B form ------
def _a_case(name):
    """(genes, values [T, N], P, the permutations held to the restatement)."""
    if name == "tails":                     # N = 257, T = 3, P = 70: a K tail, a second chunk, a ragged second stage
        genes, vals, P, _ = _values("tails")
        return genes, vals, P, (0, 31, 32, 63, 64, 69)
    if name == "distinct":                  # N = 2100, P = 33: nine chunks, negative hi digits, one column of tile 1
        genes, vals, P, _ = _values("distinct")
        return genes, vals, P, (0, 1, 31, 32)
    assert name == "one"                    # one permutation: 63 columns of the stage are not the generator's
    rng = np.random.default_rng(331)
    vals = np.round(rng.standard_normal((1, 33)), 1)
    vals[0, [2, 30]] = np.nan
    return _genes(rng, 70, 33), vals, 1, (0,)


@pytest.mark.parametrize("name", ("tails", "one", "distinct"))
def test_generated_b_operand_byte_for_byte(eng, name):
    genes, vals, P, sample = _a_case(name)
    T, N = vals.shape
    plan = eng.ranksum_plan(vals)
    dev = _gen_bfrag(eng, plan.rc, plan.valid, T, N, P)
    buf = dev.cpu().numpy()
    rows = _gen_rows(eng, plan.rc, plan.valid, T, N, P)
    assert (rows != ROW_FILL).all()
    got, dig, pad, _ = rs.bfrag_decode(buf, T, P, N)
    assert np.array_equal(got, rows)
    # every byte of the columns < P, K pad included, is the encoder's -- over the device's own plain rows ...
    assert np.array_equal(rs.bfrag_unpack(buf, T, P, N)[:, :P],
                          rs.bfrag_unpack(rs.bfrag_encode(rows, N), T, P, N)[:, :P])
    assert not pad.any()
    # ... and over the restatement's rows, from the seed alone, at a sample of columns
    for t in range(T):
        valid, rc, _, _, _ = rs.ranks(vals[t].tolist())
        want = rs.bfrag_unpack(rs.bfrag_encode(_spec_rows(t, sample, valid, rc)[None], N), 1, len(sample), N)
        assert np.array_equal(rs.bfrag_unpack(buf, T, P, N)[t, list(sample)], want[0, :len(sample)]), (name, t)
    if name == "distinct":
        assert dig[..., 0].min() < -8 and dig[..., 0].max() > 8
    if name == "tails":                     # a call that starts at a permutation that is no multiple of 64
        later = _gen_bfrag(eng, plan.rc, plan.valid, T, N, P - 37, perm_base=37).cpu().numpy()
        assert np.array_equal(rs.bfrag_unpack(later, T, P - 37, N)[:, :P - 37],
                              rs.bfrag_unpack(buf, T, P, N)[:, 37:P])
    # the header leaves the columns at and past P open: the counts do not depend on them
    gm = eng.pack_dense(genes)
    d_obs = _observed(eng, gm, plan)["d"]
    r = _permute(eng, gm, dev, d_obs, T, N, P, start=R0)
    full = rs.bfrag_unpack(buf, T, P, N).copy()
    full[:, P:] = 0x7F
    assert full[:, P:].size > 0
    assert np.array_equal(_permute(eng, gm, rs.bfrag_pack(full), d_obs, T, N, P, start=R0), r)
    for t in range(T):
        assert np.array_equal(r[t], R0 + _counts(genes, rows[t], d_obs[t])[0]), (name, t)


# ---------------------------------------------------------------- b. trait_base ------
def test_trait_base_is_part_of_the_counter(eng):
    rng = np.random.default_rng(22)
    N, P = 300, 5
    row = np.round(rng.standard_normal(N), 1)
    row[rng.random(N) < 0.2] = np.nan
    vals = np.tile(row, (3, 1))                                      # three traits with identical values
    plan = eng.ranksum_plan(vals)
    valid, rc, _, _, _ = rs.ranks(row.tolist())
    all3 = _gen_rows(eng, plan.rc, plan.valid, 3, N, P)
    one = _gen_rows(eng, plan.rc, plan.valid, 1, N, P, trait_base=2)
    assert np.array_equal(one[0], all3[2]) and np.array_equal(one[0], _spec_rows(2, range(P), valid, rc))
    assert not np.array_equal(one[0], all3[0]) and not np.array_equal(all3[1], all3[0])
    assert np.array_equal(all3[0], _spec_rows(0, range(P), valid, rc))
    b3 = rs.bfrag_decode(_gen_bfrag(eng, plan.rc, plan.valid, 3, N, P).cpu().numpy(), 3, P, N)
    b1 = rs.bfrag_decode(_gen_bfrag(eng, plan.rc, plan.valid, 1, N, P, trait_base=2).cpu().numpy(), 1, P, N)
    assert np.array_equal(b1[0][0], all3[2]) and np.array_equal(b3[0], all3)
    assert np.array_equal(b1[1][0], b3[1][2]) and not b1[2].any() and not b3[2].any()
    assert not np.array_equal(b1[0][0], b3[0][0])


# ---------------------------------------------------------------- c. edge traits ------
def _edge_case(N):
    """values [T, N] and P: the traits spec'd for this N."""
    rng = np.random.default_rng(1000 + N)

    def trait(idx, values):
        x = np.full(N, np.nan)
        x[np.asarray(idx, dtype=int)] = values
        return x

    def subset(n):                                                   # n valid isolates, the last one among them
        idx = rng.permutation(N - 1)[:n - 1]
        return trait(np.append(idx, N - 1), rng.permutation(n) * 0.5 - 3.0)

    if N == 1:
        return np.stack([trait([0], 4.0), trait([], [])]), 3
    if N in (31, 32, 33, 256):
        two = rng.permutation(N)[:2]
        return np.stack([trait([], []),                              # n = 0
                         trait([N - 1], 1.5),                        # n = 1
                         trait([0, N - 1], [2.0, -1.0]),             # n = 2, distinct
                         trait(two, [7.0, 7.0]),                     # n = 2, tied: f = 0
                         np.round(rng.standard_normal(N), 1)]), 3    # n = N, some ties
    if N == 1100:
        return np.stack([subset(1024), subset(1025)]), 3
    if N == 600:
        return np.stack([subset(512), subset(513)]), 3
    assert N in (4096, 4097)
    return (rng.permutation(N) * 0.25 - 100.0)[None], 2


@pytest.mark.parametrize("N", (1, 31, 32, 33, 256, 600, 1100, 4096, 4097))
def test_edge_traits_through_all_three_kernels(eng, N):
    vals, P = _edge_case(N)
    T, G = len(vals), 70
    genes = _genes(np.random.default_rng(N), G, N)
    fresh = N == 4097              # the generator's first launch on its handle is the one that needs the LDS opt-in
    if fresh:
        from scoary_amd.engine import AssociationEngine
        e = AssociationEngine(0)
    else:
        e = eng
    try:
        plan = e.ranksum_plan(vals)
        rows = _gen_rows(e, plan.rc, plan.valid, T, N, P)
        bfrag = _gen_bfrag(e, plan.rc, plan.valid, T, N, P)
        gm = e.pack_dense(genes)
        res = _observed(e, gm, plan)
        r = _permute(e, gm, bfrag, res["d"], T, N, P, start=R0)
        buf = bfrag.cpu().numpy()
    finally:
        if fresh:
            e.close()
    got, _, pad, _ = rs.bfrag_decode(buf, T, P, N)
    assert np.array_equal(got, rows) and not pad.any()
    untestable, worst = 0, 0.0
    for t in range(T):
        valid, rc, n, tiesum, _ = rs.ranks(vals[t].tolist())
        assert np.array_equal(plan.rc_host[t], np.asarray(rc)) and plan.n[t] == n and plan.tiesum_host[t] == tiesum
        assert np.array_equal(plan.valid_host[t], np.asarray(valid, dtype=bool))
        D = genes.astype(np.int64) @ np.asarray(rc, dtype=np.int64)
        m = genes.astype(np.int64) @ np.asarray(valid, dtype=np.int64)
        for g in (0, 3, G - 1):
            assert (int(D[g]), int(m[g])) == rs.statistic(genes[g].tolist(), valid, rc)
        assert np.array_equal(res["d"][t], D) and np.array_equal(res["m"][t], m), (N, t)
        spec = _spec_rows(t, range(P), valid, rc)
        assert np.array_equal(rows[t], spec), (N, t)
        want = _counts(genes, spec, D)[0]
        few = [0, 1, 2, 3, G - 1]
        assert rs.r_q([genes[g].tolist() for g in few], spec.tolist(), [int(D[g]) for g in few]) == want[few].tolist()
        assert np.array_equal(r[t], R0 + want), (N, t)
        for g in range(G):
            ok, auc, p = rs.tail(int(D[g]), int(m[g]), n, tiesum)
            assert res["auc"][t, g] == auc, (N, t, g)
            if not ok:
                untestable += 1
                assert D[g] == 0 and res["p"][t, g] == 1.0 and auc == 0.5 and r[t, g] == R0 + P, (N, t, g)
            else:
                assert p > 0
                worst = max(worst, abs(res["p"][t, g] - p) / p)
    print("N = %d: %d untestable of %d, max relative p difference %.3g" % (N, untestable, T * G, worst))
    assert worst <= 1e-10 and untestable >= 2 * T


# ---------------------------------------------------------------- d. stage boundary, several K chunks ------
def test_stages_per_block_with_several_k_chunks_and_a_ragged_last_range(eng):
    """k_permute_ranksum where a block serves several stages of several K chunks each: at a stage boundary the chunk
    of the gene bits starts again at 0 while B runs straight on, the last range has fewer stages than the others,
    and the trait offset of B is not zero.  N = 520: three chunks over the six quads of the tiled matrix, five of
    which hold isolates.  (Row sizes come from a fixed list and no size past one quad is odd, so the kernel's clamp
    to the last quad is only reached where the matrix is one quad and one chunk, N <= 128: the small cases of
    test_edge_traits_through_all_three_kernels.)  The shape follows the launch rule of scoary_permute_ranksum for
    the device found, and the test fails if the launch would not enter the path.  B is the test's own (bfrag_encode
    of random rows), the thresholds are |D| of a random column of each gene, so equality occurs in every gene."""
    import torch
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    T, P, N = 8, 1070, 520
    nblk = max(2, -(-16 * cus // (8 * T)))                       # want = 8 of the S = 17 stages: L = 3
    G = nblk * 256 - 100
    S = -(-P // 64)
    want = min(S, max(1, -(-16 * cus // (nblk * T))))            # the launch rule, copied
    L = -(-S // want)
    ranges, nc = -(-S // L), rs.chunks(N)
    print("CUs %d: T %d G %d (%d blocks) P %d S %d want %d L %d ranges %d last range %d stages, nc %d, quads %d"
          % (cus, T, G, nblk, P, S, want, L, ranges, S - (ranges - 1) * L, nc, eng.quads(N)))
    assert L >= 2 and S % L != 0 and T >= 2 and nblk >= 2 and G % 256 != 0 and P % 64 not in (0, 32)
    assert nc >= 2 and eng.quads(N) == 2 * nc
    rng = np.random.default_rng(520)
    rows = rng.integers(-16319, 16320, (T, P, N))
    for t in range(T):
        rows[t][:, rng.random(N) < 0.1] = 0                      # the trait's invalid isolates
    rows[:, :, N - 1] = rng.integers(1, 16320, (T, P))           # the last isolate counts
    genes = _genes(rng, G, N)
    gm = eng.pack_dense(genes)
    col = rng.integers(0, P, (T, G))
    sign = rng.choice([-1, 1], (T, G))
    thr = np.empty((T, G), dtype=np.int64)
    counts = np.empty((T, G), dtype=np.int64)
    g64 = genes.astype(np.float64)
    for t in range(T):
        D = g64 @ rows[t].astype(np.float64).T                   # exact: integers below 2^53
        thr[t] = np.abs(D[np.arange(G), col[t]]).astype(np.int64) * sign[t]
        counts[t] = (np.abs(D) >= np.abs(thr[t])[:, None]).sum(axis=1)
    assert counts.min() >= 1 and (counts[:, 1] == P).all() and (thr < 0).any() and (thr > 0).any()
    assert len(np.unique(counts)) > P // 2                       # the counts spread over [1, P]
    few = [0, 255, 256, G // 2, G - 1]
    t = T - 1
    assert rs.r_q([genes[g].tolist() for g in few], rows[t].tolist(), [int(thr[t, g]) for g in few]) == \
        counts[t, few].tolist()
    r = _permute(eng, gm, rs.bfrag_encode(rows, N), thr, T, N, P, start=R0)
    bad = np.argwhere(r != R0 + counts)
    assert len(bad) == 0, "%d of %d cells differ, first (t, g) %s" % (len(bad), T * G, bad[:5].tolist())


# ---------------------------------------------------------------- e. |D| per cell ------
def test_exact_sums_per_cell_up_to_the_largest_the_contract_allows(eng):
    """The rank-sum counterpart of probe_regions.py: a B operand in which six columns alone are non-zero, and
    thresholds walked over the expected |D| of each of them.  A launch with d_dobs = E counts the columns with
    |D| >= E, one with E + 1 those with |D| >= E + 1; both equal to numpy's int64 count at E = |D[g][c]| for every
    chosen column c pins |D[g][c]| itself.  N = 16 320: the all-ones gene under the column of +16 319 gives
    16 320 x 16 319 = 266 326 080, the largest sum the digit split has to carry."""
    N, G, P = rs.MAX_ISOLATES, 40, 70
    chosen = (0, 31, 32, 63, 64, 69)
    rng = np.random.default_rng(16320)
    rows = np.zeros((1, P, N), dtype=np.int64)
    rows[0, 0] = 16319
    rows[0, 31] = -16319
    rows[0, 32] = 16319 * (1 - 2 * (np.arange(N) & 1))           # alternating signs
    rows[0, 63] = 127 * 128 - 64                                 # lo digit -64 everywhere
    rows[0, 64] = -127 * 128 + 63                                # lo digit 63 everywhere
    rows[0, 69, N - 1] = -16319                                  # one isolate, the last
    assert {rs.digits(int(rows[0, 63, 0]))[1], rs.digits(int(rows[0, 64, 0]))[1]} == {-64, 63}
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[0] = 1
    genes[1] = 0
    genes[2] = np.arange(N) & 1
    genes[3] = 0
    genes[3, N - 1] = 1
    D = genes.astype(np.int64) @ rows[0].T                       # [G, P], int64
    assert D[0, 0] == 266326080 == -D[0, 31] and D[2, 32] == -16319 * (N // 2) and D[3, 69] == -16319
    gm = eng.pack_dense(genes)
    bfrag = _dev(eng, rs.bfrag_encode(rows, N))

    def launch(thr):
        want = R0 + (np.abs(D) >= np.abs(thr)[:, None]).sum(axis=1)
        got = _permute(eng, gm, bfrag, thr, 1, N, P, start=R0)[0]
        assert np.array_equal(got, want), (thr.tolist(), got.tolist(), want.tolist())
        return got - R0

    for c in chosen:
        E = np.abs(D[:, c])
        at, above = launch(E), launch(E + 1)
        assert (at >= 1).all() and (above < at).all()            # column c itself is in the one and not the other
    assert (launch(-np.abs(D[:, 0])) >= 1).all()                 # a negative threshold counts as its absolute value
    assert (launch(np.zeros(G, dtype=np.int64)) == P).all()      # |D| >= 0: every column < P, none past it
    assert launch(np.full(G, 266326081))[0] == 0 and launch(np.full(G, 266326080))[0] == 2


# ---------------------------------------------------------------- f. the deep tail of p ------
def test_p_of_a_driver_gene_down_to_the_underflow(eng):
    """All values distinct and the gene = "value above the median": z grows like sqrt(3 n) / 2, and the p of
    erfc(z / sqrt 2) leaves the normal range of doubles between n = 1800 and n = 2100.  Where the restatement's p is
    normal: 1e-10 relative, as everywhere in this suite (erfc's condition number at x = z / sqrt 2 is about 2 x^2,
    at most about 1420 before underflow, so a few ulps of z cost under 1e-12).  Below 2.2250738585072014e-308 each
    side rounds to the subnormal grid once: 1e-10 relative plus two grid steps.  Where it is 0.0, 0.0."""
    N = 2100
    sub = [n for n in range(1800, 2101)
           if 0.0 < rs.tail((n // 2) * (n - n // 2), n // 2, n, 0)[2] < DBL_MIN]
    assert sub and rs.tail(1050 * 1050, 1050, 2100, 0)[2] == 0.0
    ns = [600, 1000, 1800, sub[0], sub[len(sub) // 2], N]
    rng = np.random.default_rng(6)
    vals = np.full((len(ns), N), np.nan)
    genes = np.zeros((len(ns), N), dtype=np.uint8)
    for t, n in enumerate(ns):
        idx = rng.permutation(N)[:n]
        vals[t, idx] = rng.permutation(n) * 0.5
        genes[t, idx] = vals[t, idx] > np.median(vals[t, idx])
    plan = eng.ranksum_plan(vals)
    res = _observed(eng, eng.pack_dense(genes), plan)
    seen = set()
    for t, n in enumerate(ns):
        valid, rc, n_, tiesum, _ = rs.ranks(vals[t].tolist())
        assert n_ == n and tiesum == 0
        for g in range(len(ns)):
            D, m = rs.statistic(genes[g].tolist(), valid, rc)
            assert (res["d"][t, g], res["m"][t, g]) == (D, m)
            ok, auc, p = rs.tail(D, m, n, tiesum)
            got = float(res["p"][t, g])
            assert ok and res["auc"][t, g] == auc
            kind = "zero" if p == 0.0 else "subnormal" if p < DBL_MIN else "normal"
            if g == t:
                assert m == n // 2 and D == m * (n - m) and auc == 1.0
                seen.add(kind)
                print("n = %d: p %.17g, restatement %.17g (%s), difference %.3g"
                      % (n, got, p, kind, abs(got - p) / p if p else abs(got - p)))
            if kind == "zero":
                assert got == 0.0, (n, g, got)
            elif kind == "subnormal":
                assert abs(got - p) <= 1e-10 * p + 2 * 4.94e-324, (n, g, got, p)
            else:
                assert abs(got - p) <= 1e-10 * p, (n, g, got, p)
    assert seen == {"normal", "subnormal", "zero"}
