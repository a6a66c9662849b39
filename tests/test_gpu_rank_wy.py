"""Westfall-Young single-step maxT over the rank statistics (spec S17) on the GPU, through the raw entry points and
the engine, against the restatement rank_wy_spec.py: var, iv, s_obs, maxs and r_fwer bit for bit, d_r bit for bit
what scoary_permute_ranksum returns.  The permuted statistics of the reference are int64 products of the gene rows
with the rows the generators write in plain form (ranksum_values / vanelteren_values: held to the restatements of
S15 / S16 by those specs' own tests), or with rows the test makes itself.

Shapes: G at the edges of a block of 256 genes; N at the edges of a word, a chunk and the generator's 64 KB of LDS,
and the largest, 16 320; P at the edges of a column tile and of a stage of 64, with the B operand's pad columns full
of 0x7f bytes and sentinels behind the P columns of maxs; a block that walks three stages with a ragged last range;
traits that cannot be tested; maxs that starts above zero; two batches against one; S16 with nine strata, and with
one stratum against the S15 rows."""
import ctypes

import numpy as np
import pytest

import rank_wy_spec as wy
import ranksum_spec as rs
import vanelteren_spec as ve

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE1234567
R0 = 5                               # where d_r starts: batches add up
ERR_ARG, ERR_SIZE = -1, -3           # SCOARY_ERR_ARG, SCOARY_ERR_SIZE of include/scoary_hip.h
SENTINEL = 123.4375                  # behind the P columns of maxs


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _genes(rng, G, N):
    """Random densities, plus the empty, the full and the last-isolate-only gene where there is room."""
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    if G > 3:
        genes[1] = 0
        genes[2] = 1
        genes[3] = 0
        genes[3, N - 1] = 1
    return genes


def _values(rng, T, N):
    """Trait 0 with ties and missing values, the others distinct."""
    vals = rng.permutation(T * N).reshape(T, N) * 0.25 - 7.0
    vals[0] = np.round(rng.standard_normal(N), 1)
    if N > 2:
        vals[0, rng.random(N) < 0.2] = np.nan
        vals[0, N - 1] = 0.5                                         # the last isolate counts
    return vals


def _ranksum_bfrag(eng, plan, P, perm_base=0):
    """The S15 generator's B operand in a buffer that held 0x7f bytes: the pad columns keep them."""
    import torch
    buf = torch.full((int(eng.lib.scoary_ranksum_bfrag_bytes(plan.N, P, plan.T)),), 0x7F, dtype=torch.uint8,
                     device=eng.device)
    eng._check(eng.lib.scoary_ranksum_perm_generate_bfrag(
        eng.h, eng._ptr(plan.rc), eng._ptr(plan.valid), plan.T, plan.N, P, perm_base, 0, ctypes.c_uint64(SEED),
        eng._ptr(buf), eng._stream()), "scoary_ranksum_perm_generate_bfrag")
    return buf


def _count_pass(eng, gm, bfrag, dobs, T, N, P):
    """scoary_permute_ranksum onto a d_r that holds R0 -> int32 [T, G] on the host."""
    import torch
    r = torch.full((T, gm.G), R0, dtype=torch.int32, device=eng.device)
    eng._check(eng.lib.scoary_permute_ranksum(eng.h, eng._ptr(gm.tiled), eng._ptr(bfrag), eng._ptr(dobs), gm.G, T, N,
                                              P, eng._ptr(r), eng._stream()), "scoary_permute_ranksum")
    return r.cpu().numpy()


def _maxt_pass(eng, gm, bfrag, dobs, iv, cc, T, N, P, start=None, tail=7):
    """scoary_permute_rank_wy onto a d_r that holds R0 and a maxs [T, P + tail] that holds `start` (default zeros) in
    its first P columns and SENTINEL behind them -> (r int32 [T, G], maxs float64 [T, P + tail]) on the host."""
    import torch
    stride = P + tail
    mx = np.full((T, stride), SENTINEL)
    mx[:, :P] = 0.0 if start is None else start
    mx = _dev(eng, mx)
    r = torch.full((T, gm.G), R0, dtype=torch.int32, device=eng.device)
    eng._check(eng.lib.scoary_permute_rank_wy(
        eng.h, eng._ptr(gm.tiled), eng._ptr(bfrag), eng._ptr(dobs), eng._ptr(iv), cc, gm.G, T, N, P, eng._ptr(r),
        eng._ptr(mx), stride, eng._stream()), "scoary_permute_rank_wy")
    return r.cpu().numpy(), mx.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _products(genes, rows):
    """D int64 [T, G, P] of the gene rows against rows int [T, P, N]."""
    g = genes.astype(np.int64)
    return np.stack([g @ rows[t].astype(np.int64).T for t in range(rows.shape[0])])


def _ranksum_reference(genes, vals):
    """Per trait the restatement's (d, m, var, iv, s_obs) as arrays [T, G]; n and tiesum from ranksum_spec.ranks."""
    out = {k: [] for k in ("d", "m", "var", "iv", "s_obs")}
    for t in range(vals.shape[0]):
        valid, rc, n, tiesum, _ = rs.ranks(vals[t].tolist())
        d = genes.astype(np.int64) @ np.asarray(rc, dtype=np.int64)
        m = genes.astype(np.int64) @ np.asarray(valid, dtype=np.int64)
        var = np.asarray([wy.var_ranksum(int(x), n, tiesum) for x in m])
        iv = np.asarray([wy.inverse(v) for v in var])
        for k, v in (("d", d), ("m", m), ("var", var), ("iv", iv), ("s_obs", wy.stats(d, 1, iv))):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def _check_ranksum_shape(eng, G, N, P, T=2, seed=0):
    """One shape through the raw entry points, everything bit for bit; returns what the callers look at."""
    rng = np.random.default_rng(1000 * G + 10 * N + P + seed)
    genes, vals = _genes(rng, G, N), _values(rng, T, N)
    ref = _ranksum_reference(genes, vals)
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    assert np.array_equal(res["d"].cpu().numpy(), ref["d"]) and np.array_equal(res["m"].cpu().numpy(), ref["m"])
    var = eng.ranksum_var(plan, res["m"])
    iv, sobs = eng.rank_wy_prepare(var, res["d"], 1)
    assert _same_bits(var.cpu().numpy(), ref["var"]), (G, N, P)
    assert _same_bits(iv.cpu().numpy(), ref["iv"]), (G, N, P)
    assert _same_bits(sobs.cpu().numpy(), ref["s_obs"]), (G, N, P)
    bfrag = _ranksum_bfrag(eng, plan, P)
    if P % 64:
        pad = rs.bfrag_unpack(bfrag.cpu().numpy(), T, P, N)[:, P:]
        assert pad.size and (pad == 0x7F).all()                      # the pad columns hold large values
    rows = eng.ranksum_values(plan, 0, P, SEED).cpu().numpy()
    D = _products(genes, rows)
    r, mx = _maxt_pass(eng, gm, bfrag, res["d"], iv, 1, T, N, P)
    assert np.array_equal(r, _count_pass(eng, gm, bfrag, res["d"], T, N, P)), (G, N, P)
    want_r = np.stack([wy.r_count(D[t], ref["d"][t]) for t in range(T)])
    assert np.array_equal(r, R0 + want_r), (G, N, P)
    want_mx = np.stack([wy.maxs(D[t], 1, ref["iv"][t]) for t in range(T)])
    assert (mx[:, P:] == SENTINEL).all(), (G, N, P)
    bad = np.argwhere(mx[:, :P].view(np.uint64) != want_mx.view(np.uint64))
    assert len(bad) == 0, "(G %d, N %d, P %d): %d of %d maxima differ, first (t, p) %s" % (
        G, N, P, len(bad), T * P, bad[:5].tolist())
    rf = eng.r_fwer_max(_dev(eng, mx[:, :P]), sobs).cpu().numpy()
    want_rf = np.stack([wy.r_fwer(want_mx[t], ref["s_obs"][t]) for t in range(T)])
    assert np.array_equal(rf, want_rf) and (rf >= want_r).all(), (G, N, P)
    capped = (ref["iv"] == 0) | (np.abs(ref["d"]) <= 1)
    assert (rf[capped] == P).all()
    if G == 1:
        assert np.array_equal(rf, want_r)
    return ref, want_mx, rf


# ---------------------------------------------------------------- 1. block, word, chunk, tile and stage edges ------
@pytest.mark.parametrize("G, N, P", ((1, 33, 1), (255, 31, 63), (256, 256, 64), (257, 257, 65), (513, 1, 130),
                                     (1, 257, 130), (255, 33, 65), (513, 256, 63), (70, 4097, 65)))
def test_shapes_bit_for_bit(eng, G, N, P):
    ref, mx, rf = _check_ranksum_shape(eng, G, N, P)
    if N == 1:
        assert not ref["iv"].any() and not mx.any() and (rf == P).all()     # no trait of one isolate can be tested
    elif G > 1:
        assert (ref["iv"] > 0).any() and (mx > 0).all()


def test_the_largest_matrix_and_the_gene_of_the_positive_ranks(eng):
    """N = 16 320, all values distinct: gene 0 carries exactly the isolates of positive Rc, so its D is the largest
    sum real ranks give (n^2 / 4 = 66 585 600); then columns the test writes itself, where the all-ones gene reaches
    |D| = 266 326 080 and E^2 needs more than 53 bits."""
    G, N, P, T = 8, rs.MAX_ISOLATES, 64, 1
    rng = np.random.default_rng(16320)
    vals = (rng.permutation(N) * 1.0)[None]
    genes = _genes(rng, G, N)
    _valid, rc, _n, _ts, _ = rs.ranks(vals[0].tolist())
    genes[0] = np.asarray(rc) > 0
    ref = _ranksum_reference(genes, vals)
    assert ref["d"][0, 0] == (N // 2) ** 2 == 66585600
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    var = eng.ranksum_var(plan, res["m"])
    iv, sobs = eng.rank_wy_prepare(var, res["d"], 1)
    assert _same_bits(iv.cpu().numpy(), ref["iv"]) and _same_bits(sobs.cpu().numpy(), ref["s_obs"])
    bfrag = _ranksum_bfrag(eng, plan, P)
    D = _products(genes, eng.ranksum_values(plan, 0, P, SEED).cpu().numpy())
    r, mx = _maxt_pass(eng, gm, bfrag, res["d"], iv, 1, T, N, P)
    assert np.array_equal(r, _count_pass(eng, gm, bfrag, res["d"], T, N, P))
    assert np.array_equal(r[0], R0 + wy.r_count(D[0], ref["d"][0]))
    assert _same_bits(mx[0, :P], wy.maxs(D[0], 1, ref["iv"][0])) and (mx[:, P:] == SENTINEL).all()
    rf = eng.r_fwer_max(_dev(eng, mx[:, :P]), sobs).cpu().numpy()
    assert np.array_equal(rf[0], wy.r_fwer(mx[0, :P], ref["s_obs"][0])) and rf[0, 0] == 0 and r[0, 0] == R0
    # the same gene against columns the test writes: |D| at the largest the digit split carries, both signs
    rows = np.zeros((1, P, N), dtype=np.int64)
    rows[0, 0], rows[0, 33] = 16319, -16319
    rows[0, 63, N - 1] = 7
    genes[4] = 1
    gm = eng.pack_dense(genes)
    D = _products(genes, rows)
    assert D[0, 4, 0] == wy.MAX_E == -D[0, 4, 33] and wy.MAX_E ** 2 > 2 ** 53
    ivs = np.linspace(1e-9, 3e-7, G)[None]
    thr = _dev(eng, np.full((1, G), 12345, dtype=np.int32))
    for cc in (0, 1):
        _r, mx = _maxt_pass(eng, gm, _dev(eng, rs.bfrag_encode(rows, N)), thr, _dev(eng, ivs), cc, 1, N, P)
        assert _same_bits(mx[0, :P], wy.maxs(D[0], cc, ivs[0])) and mx[0, 0] == mx[0, 33] > 0 and mx[0, 1] == 0


# ---------------------------------------------------------------- 2. several stages per block ------
def test_three_stages_per_block_with_a_ragged_last_range(eng):
    """The shape of test_gpu_ranksum_limits' stage test, by the launch rule the two entry points share: S = 17
    stages in ranges of L = 3 with a last range of two, three K chunks per stage, T = 8 so that the trait offsets of
    B, d_iv and maxs are not zero.  B is the test's own, the thresholds are |D| of a random column of each gene, iv
    random with zeros among them, and both continuity constants go over the same B."""
    import torch
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    T, P, N = 8, 1070, 520
    nblk = max(2, -(-16 * cus // (8 * T)))
    G = nblk * 256 - 100
    S = -(-P // 64)
    want = min(S, max(1, -(-16 * cus // (nblk * T))))            # the launch rule, copied
    L = -(-S // want)
    assert L == 3 and S == 17 and S % L == 2 and G % 256 != 0 and rs.chunks(N) == 3
    rng = np.random.default_rng(521)
    rows = rng.integers(-16319, 16320, (T, P, N))
    rows[:, :, N - 1] = rng.integers(1, 16320, (T, P))
    genes = _genes(rng, G, N)
    gm = eng.pack_dense(genes)
    iv = rng.uniform(1e-9, 1e-3, (T, G))
    iv[rng.random((T, G)) < 0.1] = 0.0
    iv[:, G - 1] = 1e-3                                          # the last gene of the ragged block can win
    g64 = genes.astype(np.float64)
    thr = np.empty((T, G), dtype=np.int32)
    counts = np.empty((T, G), dtype=np.int64)
    mx = {0: np.empty((T, P)), 1: np.empty((T, P))}
    winners = set()
    for t in range(T):
        D = (g64 @ rows[t].astype(np.float64).T).astype(np.int64)    # exact: integers below 2^53
        thr[t] = np.abs(D[np.arange(G), rng.integers(0, P, G)])
        counts[t] = wy.r_count(D, thr[t])
        for cc in (0, 1):
            s = wy.stats(D, cc, iv[t])
            mx[cc][t] = s.max(axis=0)
        winners.update((s.argmax(axis=0) // 256).tolist())
    assert len(winners) > nblk // 4                              # the maxima come from many blocks
    bfrag, dthr, div = _dev(eng, rs.bfrag_encode(rows, N)), _dev(eng, thr), _dev(eng, iv)
    plain = _count_pass(eng, gm, bfrag, dthr, T, N, P)
    assert np.array_equal(plain, R0 + counts)
    for cc in (0, 1):
        r, got = _maxt_pass(eng, gm, bfrag, dthr, div, cc, T, N, P)
        assert np.array_equal(r, plain)
        bad = np.argwhere(got[:, :P].view(np.uint64) != mx[cc].view(np.uint64))
        assert len(bad) == 0, "cc %d: %d of %d maxima differ, first (t, p) %s" % (cc, len(bad), T * P, bad[:5].tolist())
        assert (got[:, P:] == SENTINEL).all()
    assert not np.array_equal(mx[0], mx[1])


# ---------------------------------------------------------------- 3. traits that cannot be tested ------
def test_untestable_traits_have_zero_maxima_and_r_fwer_p(eng):
    G, N, P = 70, 50, 70
    rng = np.random.default_rng(7)
    genes = _genes(rng, G, N)
    vals = np.stack([np.full(N, 3.0),                                # all tied: f = 0
                     np.round(rng.standard_normal(N), 1),
                     np.full(N, np.nan)])
    vals[2, 17] = 1.0                                                # n = 1
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    r, rf, mx = (x.cpu().numpy() for x in eng.ranksum_westfall_young(gm, plan, res, P, SEED))
    assert np.array_equal(r, eng.ranksum_permute(gm, plan, res["d"], P, SEED).cpu().numpy())
    assert mx.shape == (3, P) and not mx[0].any() and not mx[2].any() and (mx[1] > 0).all()
    assert (rf[0] == P).all() and (rf[2] == P).all() and (r[0] == P).all() and (r[2] == P).all()
    ref = _ranksum_reference(genes, vals)
    D = _products(genes, eng.ranksum_values(plan, 0, P, SEED).cpu().numpy())
    assert _same_bits(mx[1], wy.maxs(D[1], 1, ref["iv"][1]))
    assert np.array_equal(rf[1], wy.r_fwer(mx[1], ref["s_obs"][1])) and (rf[1] >= r[1]).all() and (rf[1] > r[1]).any()
    assert (rf[1, [1, 2]] == P).all() and rf[1].min() < P


# ---------------------------------------------------------------- 4. maxs that does not start at zero ------
def test_larger_values_in_maxs_stay(eng):
    G, N, P, T = 300, 100, 65, 2
    rng = np.random.default_rng(44)
    genes, vals = _genes(rng, G, N), _values(rng, T, N)
    ref = _ranksum_reference(genes, vals)
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    iv, _sobs = eng.rank_wy_prepare(eng.ranksum_var(plan, res["m"]), res["d"], 1)
    bfrag = _ranksum_bfrag(eng, plan, P)
    D = _products(genes, eng.ranksum_values(plan, 0, P, SEED).cpu().numpy())
    want = np.stack([wy.maxs(D[t], 1, ref["iv"][t]) for t in range(T)])
    start = np.zeros((T, P))
    start[:, ::3] = 1e300                                            # stays
    start[0, 1::3] = want[0, 1::3]                                   # equal: stays, bit for bit
    start[1, 1::3] = np.nextafter(want[1, 1::3], 0.0)                # one ulp below: replaced
    _r, mx = _maxt_pass(eng, gm, bfrag, res["d"], iv, 1, T, N, P, start=start)
    assert _same_bits(mx[:, :P], np.maximum(start, want)) and (mx[:, P:] == SENTINEL).all()
    assert (mx[:, 0] == 1e300).all() and _same_bits(mx[1, 1:P:3], want[1, 1::3])


def test_argument_checks(eng):
    import torch
    G, N, P, T = 4, 40, 3, 1
    gm = eng.pack_dense(np.ones((G, N), dtype=np.uint8))
    z = torch.zeros((T, max(G, P) + 64), dtype=torch.float64, device=eng.device)
    d = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    r = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    b = torch.zeros((int(eng.lib.scoary_ranksum_bfrag_bytes(N, P, T)),), dtype=torch.uint8, device=eng.device)

    def call(cc=1, n=N, p=P, stride=P, t=T):
        return eng.lib.scoary_permute_rank_wy(eng.h, eng._ptr(gm.tiled), eng._ptr(b), eng._ptr(d), eng._ptr(z), cc, G,
                                              t, n, p, eng._ptr(r), eng._ptr(z), stride, eng._stream())
    for kw in (dict(cc=2), dict(cc=-1), dict(stride=P - 1), dict(p=0)):
        assert call(**kw) == ERR_ARG, kw
    for kw in (dict(n=rs.MAX_ISOLATES + 1), dict(t=65536), dict(p=1 << 31, stride=1 << 31)):
        assert call(**kw) == ERR_SIZE, kw
    assert eng.lib.scoary_rank_wy_prepare(eng.h, eng._ptr(z), eng._ptr(d), 2, G, T, eng._ptr(z), eng._ptr(z),
                                          eng._stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert not r.any().item() and not z.any().item()                 # a refused call writes nothing
    assert call() == 0                                               # thresholds 0, iv 0: every column counts, s = 0
    torch.cuda.synchronize()
    assert (r == P).all().item() and not z.any().item()


# ---------------------------------------------------------------- 5. batches ------
def test_two_batches_of_64_are_one_of_128(eng):
    G, N, P, T = 300, 257, 128, 2
    rng = np.random.default_rng(128)
    genes, vals = _genes(rng, G, N), _values(rng, T, N)
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    assert eng.ranksum_batch(T, N, P, 1) == 64 and eng.ranksum_batch(T, N, P) == 128
    one = [x.cpu().numpy() for x in eng.ranksum_westfall_young(gm, plan, res, P, SEED)]
    two = [x.cpu().numpy() for x in eng.ranksum_westfall_young(gm, plan, res, P, SEED, budget_bytes=1)]
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    ref = _ranksum_reference(genes, vals)
    D = _products(genes, eng.ranksum_values(plan, 0, P, SEED).cpu().numpy())
    for t in range(T):
        assert _same_bits(one[2][t], wy.maxs(D[t], 1, ref["iv"][t]))
        assert _same_bits(one[2][t, 64:], wy.maxs(D[t][:, 64:], 1, ref["iv"][t]))       # by max over batches
        assert np.array_equal(one[1][t], wy.r_fwer(one[2][t], ref["s_obs"][t]))
        assert np.array_equal(one[0][t], wy.r_count(D[t], ref["d"][t]))
    assert np.array_equal(one[0], eng.ranksum_permute(gm, plan, res["d"], P, SEED).cpu().numpy())


# ---------------------------------------------------------------- 6. S16 ------
def _vanelteren_reference(genes, vals, st, S):
    out = {k: [] for k in ("d", "var", "iv", "s_obs")}
    for t in range(vals.shape[0]):
        pr = wy.vanelteren_problem(genes.tolist(), [float(v) for v in vals[t]], [int(s) for s in st], S)
        for k in out:
            out[k].append(np.asarray(pr[k]))
    return {k: np.stack(v) for k, v in out.items()}


def test_van_elteren_nine_strata(eng):
    """S = 9 at N = 333, strata of uneven size with one of a single isolate and one of two; P = 130 in batches of 64."""
    G, N, P, T, S = 150, 333, 130, 2, 9
    rng = np.random.default_rng(333)
    genes, vals = _genes(rng, G, N), _values(rng, T, N)
    st = rng.integers(0, S - 2, N)
    st[5], st[[50, 60]] = S - 2, S - 1
    vals[:, [5, 50, 60]] = [[1.0, 2.0, 3.0]]
    ref = _vanelteren_reference(genes, vals, st, S)
    gm = eng.pack_dense(genes)
    plan = eng.vanelteren_plan(vals, st)
    res = eng.vanelteren(gm, plan)
    assert np.array_equal(res["d"].cpu().numpy(), ref["d"]) and _same_bits(res["var"].cpu().numpy(), ref["var"])
    iv, sobs = eng.rank_wy_prepare(res["var"], res["d"], 0)
    assert _same_bits(iv.cpu().numpy(), ref["iv"]) and _same_bits(sobs.cpu().numpy(), ref["s_obs"])
    r, rf, mx = (x.cpu().numpy() for x in eng.vanelteren_westfall_young(gm, plan, res, P, SEED, budget_bytes=1))
    assert np.array_equal(r, eng.vanelteren_permute(gm, plan, res["d"], P, SEED).cpu().numpy())
    D = _products(genes, eng.vanelteren_values(plan, 0, P, SEED).cpu().numpy())
    for t in range(T):
        assert np.array_equal(r[t], wy.r_count(D[t], ref["d"][t]))
        assert _same_bits(mx[t], wy.maxs(D[t], 0, ref["iv"][t])), t
        assert np.array_equal(rf[t], wy.r_fwer(mx[t], ref["s_obs"][t]))
    assert (rf >= r).all() and (rf > r).any() and (rf[ref["iv"] == 0] == P).all() and (ref["iv"] == 0).any()
    # a few permuted rows from the seed alone: the rows the reference stands on are the restatement's
    pl = ve.plan([float(v) for v in vals[1]], [int(s) for s in st], S)
    for pi in (0, 64, 129):
        assert D[1][:, pi].tolist() == [ve.statistic(g, pl, ve.perm_row(SEED, 1, pi, pl))[0] for g in genes.tolist()]


def test_one_stratum_against_the_rank_sum_rows(eng):
    """S = 1: the scores are w Rc with one weight w, the generator is S15's, so every D is w times S15's.  The counts
    are S15's exactly.  With the continuity constant set aside (cc = 0 over S15's own B operand and var), s is the
    same real number on both paths, rounded differently: var_S16 = ((w^2 f) / 12) (m (n - m)) takes three roundings
    where var_S15 takes two, then one for iv, at most one for E^2 and one for the product on either side -- eleven
    half-ulps in all, so the maxima agree within 12 x 2^-53 relative (the maximum of two families that agree cell
    by cell within a bound agrees within it)."""
    G, N, P, T = 257, 129, 65, 1
    rng = np.random.default_rng(129)
    genes = _genes(rng, G, N)
    vals = np.round(rng.standard_normal((T, N)), 1)
    vals[0, ::9] = np.nan
    gm = eng.pack_dense(genes)
    vplan = eng.vanelteren_plan(vals, np.zeros(N, dtype=np.int64))
    vres = eng.vanelteren(gm, vplan)
    vr, vrf, vmx = (x.cpu().numpy() for x in eng.vanelteren_westfall_young(gm, vplan, vres, P, SEED))
    rplan = eng.ranksum_plan(vals)
    rres = eng.ranksum(gm, rplan)
    w = int(vplan.w[0, 0])
    assert w > 1 and np.array_equal(vres["d"].cpu().numpy(), w * rres["d"].cpu().numpy())
    iv0, sobs0 = eng.rank_wy_prepare(eng.ranksum_var(rplan, rres["m"]), rres["d"], 0)
    r0, mx0 = _maxt_pass(eng, gm, _ranksum_bfrag(eng, rplan, P), rres["d"], iv0, 0, T, N, P)
    assert np.array_equal(vr, r0 - R0)
    worst = float(np.max(np.abs(vmx - mx0[:, :P]) / mx0[:, :P]))
    print("S = 1 against S15 with cc = 0: worst relative difference of the maxima %.3g" % worst)
    assert (mx0[:, :P] > 0).all() and worst <= 12 * 2.0 ** -53
    ref = _vanelteren_reference(genes, vals, np.zeros(N, dtype=np.int64), 1)
    D = _products(genes, eng.vanelteren_values(vplan, 0, P, SEED).cpu().numpy())
    assert _same_bits(vmx[0], wy.maxs(D[0], 0, ref["iv"][0]))
    assert np.array_equal(vrf[0], wy.r_fwer(vmx[0], ref["s_obs"][0]))
