"""Westfall-Young step-down maxT over the rank statistics (spec S18) on the GPU, through the raw entry points and the
engine, against the restatement rank_sd_spec.py: the order, c by rank position, r_sd and maxs bit for bit; r is what
scoary_permute_ranksum counts and r_fwer what scoary_permute_rank_wy's route gives.  The permuted statistics of the
reference are int64 products of the gene rows with the rows the generators write in plain form, or with rows the
test makes itself (ranksum_spec.bfrag_encode).

Shapes: G at the edges of a group of 64 ranks and of a block of 256, and 513 = three blocks and nine groups; N at the
edges of a word, a chunk and the generator's LDS, and the largest, 16 320; P at the edges of a column tile and of a
stage, with 0x7f bytes in B's pad columns and sentinels behind maxs, c and r; counts that start at 5; a block of three
stages with a ragged last range; tie groups across the run, lane-half, group and block boundaries; traits that cannot
be tested; a maximum that sits in the last group only and one in the first row of the first group; two batches
against one; S16 with nine strata; the planted driver of the host test."""
import ctypes

import numpy as np
import pytest

import rank_sd_spec as sd
import rank_wy_spec as wy
import ranksum_spec as rs

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE1234567
R0 = 5                               # where r and c start: batches add up
ERR_ARG, ERR_SIZE = -1, -3           # SCOARY_ERR_ARG, SCOARY_ERR_SIZE of include/scoary_hip.h
SENTINEL = 123.4375                  # behind the P columns of maxs
GUARD = -77                          # behind the [T][G] counts: the positions from G to the padded block write nothing


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
        vals[0, N - 1] = 0.5
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


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _products(genes, rows):
    """D int64 [T, G, P] of the gene rows against rows int [T, P, N]."""
    g = genes.astype(np.int64)
    return np.stack([g @ rows[t].astype(np.int64).T for t in range(rows.shape[0])])


def _ranksum_reference(genes, vals):
    """Per trait the restatement's (d, iv, s_obs) as arrays [T, G]."""
    out = {k: [] for k in ("d", "iv", "s_obs")}
    for t in range(vals.shape[0]):
        valid, rc, n, tiesum, _ = rs.ranks(vals[t].tolist())
        d = genes.astype(np.int64) @ np.asarray(rc, dtype=np.int64)
        m = genes.astype(np.int64) @ np.asarray(valid, dtype=np.int64)
        iv = np.asarray([wy.inverse(wy.var_ranksum(int(x), n, tiesum)) for x in m])
        for k, v in (("d", d), ("iv", iv), ("s_obs", wy.stats(d, 1, iv))):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def _count_pass(eng, gm, bfrag, dobs, T, N, P):
    """scoary_permute_ranksum onto zeros -> int32 [T, G] on the host."""
    import torch
    r = torch.zeros((T, gm.G), dtype=torch.int32, device=eng.device)
    eng._check(eng.lib.scoary_permute_ranksum(eng.h, eng._ptr(gm.tiled), eng._ptr(bfrag), eng._ptr(dobs), gm.G, T, N,
                                              P, eng._ptr(r), eng._stream()), "scoary_permute_ranksum")
    return r.cpu().numpy()


def _maxt_pass(eng, gm, bfrag, dobs, iv, cc, T, N, P):
    """scoary_permute_rank_wy onto zeros -> (r int32 [T, G], maxs float64 [T, P]) on the host."""
    import torch
    mx = torch.zeros((T, P), dtype=torch.float64, device=eng.device)
    r = torch.zeros((T, gm.G), dtype=torch.int32, device=eng.device)
    eng._check(eng.lib.scoary_permute_rank_wy(
        eng.h, eng._ptr(gm.tiled), eng._ptr(bfrag), eng._ptr(dobs), eng._ptr(iv), cc, gm.G, T, N, P, eng._ptr(r),
        eng._ptr(mx), P, eng._stream()), "scoary_permute_rank_wy")
    return r.cpu().numpy(), mx.cpu().numpy()


def _sd_pass(eng, gm, order, sobs, iv, dobs, bfrag, cc, N, P, perm_base=0, before=0, tail=7):
    """The gather and the three launches through the raw entry points.  r and c start at R0 and have 256 cells of
    GUARD behind them, which must stay; maxs is [T, before + P + tail] full of SENTINEL, the batch's columns are
    before .. before + P - 1 (perm_base = before).  Host arrays in, (r_rank, c_rank int32 [T, G], maxs float64
    [T, stride]) out."""
    import torch
    T, G = dobs.shape
    d_order, d_sobs, d_iv, d_dobs = (_dev(eng, x) for x in (order.astype(np.int32), sobs, iv, dobs.astype(np.int32)))
    scratch = eng.rank_stepdown_gather(gm, d_order, d_sobs, d_iv, d_dobs, N, P)
    r = torch.full((T * G + 256,), GUARD, dtype=torch.int32, device=eng.device)
    c = torch.full((T * G + 256,), GUARD, dtype=torch.int32, device=eng.device)
    r[:T * G], c[:T * G] = R0, R0
    mx = torch.full((T, before + P + tail), SENTINEL, dtype=torch.float64, device=eng.device)
    eng.permute_rank_stepdown(scratch, bfrag, cc, G, T, N, P, before, r, c, mx)
    r, c = r.cpu().numpy(), c.cpu().numpy()
    assert (r[T * G:] == GUARD).all() and (c[T * G:] == GUARD).all()
    return r[:T * G].reshape(T, G), c[:T * G].reshape(T, G), mx.cpu().numpy()


def _check_against_spec(eng, genes, D, dobs, iv, sobs, bfrag, cc, N, P, what):
    """One problem through the raw entry points, everything bit for bit; D int64 [T, G, P].  Returns the per-trait
    restatements and (r, r_sd, r_fwer) by gene."""
    T, G = dobs.shape
    gm = eng.pack_dense(genes)
    ref = [sd.stepdown(D[t], cc, iv[t], sobs[t]) for t in range(T)]
    order32, ss = eng.rank_stepdown_order(_dev(eng, sobs))
    order = order32.cpu().numpy()
    assert np.array_equal(order, np.stack([x["order"] for x in ref])), what        # one stable descending sort
    assert _same_bits(ss.cpu().numpy(), np.stack([x["ss"] for x in ref]))
    r_rank, c_rank, mx = _sd_pass(eng, gm, order, sobs, iv, dobs, bfrag, cc, N, P)
    want_r = np.stack([wy.r_count(D[t], dobs[t]) for t in range(T)])
    want_mx = np.stack([wy.maxs(D[t], cc, iv[t]) for t in range(T)])
    for t in range(T):
        bad = np.flatnonzero(c_rank[t] != R0 + ref[t]["c"])
        assert len(bad) == 0, "%s, trait %d: c differs at %d of %d ranks, first %s: got %s, want %s" % (
            what, t, len(bad), G, bad[:5].tolist(), (c_rank[t][bad[:5]] - R0).tolist(), ref[t]["c"][bad[:5]].tolist())
        assert np.array_equal(r_rank[t], R0 + want_r[t][order[t]]), (what, t)
        assert _same_bits(mx[t, :P], ref[t]["u"][0]) and _same_bits(mx[t, :P], want_mx[t]), (what, t)
    assert (mx[:, P:] == SENTINEL).all(), what
    # by gene: r is scoary_permute_ranksum's, r_fwer scoary_permute_rank_wy's route, r_sd the engine's tail
    d_dobs, d_iv = _dev(eng, dobs.astype(np.int32)), _dev(eng, iv)
    r = np.empty_like(want_r)
    np.put_along_axis(r, order.astype(np.int64), (r_rank - R0).astype(np.int64), axis=1)
    assert np.array_equal(r, _count_pass(eng, gm, bfrag, d_dobs, T, N, P)), what
    r_wy, mx_wy = _maxt_pass(eng, gm, bfrag, d_dobs, d_iv, cc, T, N, P)
    assert np.array_equal(r, r_wy) and _same_bits(mx[:, :P], mx_wy), what
    rf = eng.r_fwer_max(_dev(eng, mx_wy), _dev(eng, sobs)).cpu().numpy()
    assert np.array_equal(rf, eng.r_fwer_max(_dev(eng, mx[:, :P]), _dev(eng, sobs)).cpu().numpy())
    rsd = eng.rank_stepdown_tail(_dev(eng, c_rank - R0), ss, order32).cpu().numpy()
    assert np.array_equal(rsd, np.stack([x["r_sd"] for x in ref])), what
    return ref, r, rsd, rf


def _check_ranksum_shape(eng, G, N, P, T=2, seed=0, genes=None, vals=None):
    rng = np.random.default_rng(1000 * G + 10 * N + P + seed)
    genes = _genes(rng, G, N) if genes is None else genes
    vals = _values(rng, T, N) if vals is None else vals
    ref = _ranksum_reference(genes, vals)
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    iv, sobs = eng.rank_wy_prepare(eng.ranksum_var(plan, res["m"]), res["d"], 1)
    assert np.array_equal(res["d"].cpu().numpy(), ref["d"])
    assert _same_bits(iv.cpu().numpy(), ref["iv"]) and _same_bits(sobs.cpu().numpy(), ref["s_obs"])
    bfrag = _ranksum_bfrag(eng, plan, P)
    if P % 64:
        pad = rs.bfrag_unpack(bfrag.cpu().numpy(), T, P, N)[:, P:]
        assert pad.size and (pad == 0x7F).all()                      # the pad columns hold large values
    D = _products(genes, eng.ranksum_values(plan, 0, P, SEED).cpu().numpy())
    out = _check_against_spec(eng, genes, D, ref["d"], ref["iv"], ref["s_obs"], bfrag, 1, N, P, (G, N, P))
    return (ref,) + out


# ---------------------------------------------------------------- 1. group, block, word, chunk, tile and stage edges --
@pytest.mark.parametrize("G, N, P", ((1, 33, 1), (63, 1, 63), (64, 33, 64), (65, 4097, 65), (255, 33, 130),
                                     (256, 257, 64), (257, 257, 65), (513, 257, 130), (513, 33, 1)))
def test_shapes_bit_for_bit(eng, G, N, P):
    ref, _sdref, r, rsd, rf = _check_ranksum_shape(eng, G, N, P)
    assert (r <= rsd).all() and (rsd <= rf).all()
    capped = (ref["iv"] == 0) | (np.abs(ref["d"]) <= 1)
    assert (rsd[capped] == P).all()
    top = ref["s_obs"] == ref["s_obs"].max(axis=1, keepdims=True)
    assert np.array_equal(rsd[top], rf[top])
    if G == 1:
        assert np.array_equal(r, rsd) and np.array_equal(rsd, rf)
    if N == 1:
        assert not ref["iv"].any() and (rsd == P).all()              # no trait of one isolate can be tested


def test_the_largest_matrix_and_the_all_ones_gene(eng):
    """N = 16 320 with columns the test writes itself: the all-ones gene reaches |D| = 266 326 080, where E^2 needs
    more than 53 bits, under both signs; thresholds, iv and s_obs are the test's own, both continuity constants."""
    G, N, P = 8, rs.MAX_ISOLATES, 64
    rng = np.random.default_rng(16320)
    genes = _genes(rng, G, N)
    genes[4] = 1
    rows = np.zeros((1, P, N), dtype=np.int64)
    rows[0, 0], rows[0, 33] = 16319, -16319
    rows[0, 63, N - 1] = 7
    rows[0, 5, ::3] = 11
    D = _products(genes, rows)
    assert D[0, 4, 0] == wy.MAX_E == -D[0, 4, 33] and wy.MAX_E ** 2 > 2 ** 53
    ivs = np.linspace(1e-9, 3e-7, G)[None]
    dobs = np.full((1, G), 12345, dtype=np.int64)
    bfrag = _dev(eng, rs.bfrag_encode(rows, N))
    for cc in (0, 1):
        s = wy.stats(D[0], cc, ivs[0])
        sobs = np.sort(s[:, 5])[None]                                # observed values that the columns can reach
        sobs[0, 4] = s[4, 0]                                         # ... and the largest statistic there is
        ref, _r, _rsd, _rf = _check_against_spec(eng, genes, D, dobs, ivs, sobs, bfrag, cc, N, P, ("largest", cc))
        assert ref[0]["order"][0] == 4 and ref[0]["c"][0] == 2 and ref[0]["u"][0, 0] == ref[0]["u"][0, 33] > 0


# ---------------------------------------------------------------- 2. several stages per block ------
def test_three_stages_per_block_with_a_ragged_last_range(eng):
    """The shape of test_gpu_rank_wy's stage test, by the launch rule the entry points share: S = 17 stages in ranges
    of L = 3 with a last range of two, three K chunks per stage, T = 8 so that the trait offsets of B, the scratch and
    maxs are not zero.  B is the test's own; thresholds, iv and s_obs are random with zeros and ties among them; both
    continuity constants go over the same B."""
    import torch
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    T, P, N = 8, 1070, 520
    nblk = max(2, -(-16 * cus // (8 * T)))
    G = nblk * 256 - 100
    S = -(-P // 64)
    want = min(S, max(1, -(-16 * cus // (nblk * T))))            # the launch rule, copied
    L = -(-S // want)
    assert L == 3 and S == 17 and S % L == 2 and G % 256 != 0 and rs.chunks(N) == 3
    rng = np.random.default_rng(1818)
    rows = rng.integers(-16319, 16320, (T, P, N))
    rows[:, :, N - 1] = rng.integers(1, 16320, (T, P))
    genes = _genes(rng, G, N)
    gm = eng.pack_dense(genes)
    iv = rng.uniform(1e-9, 1e-3, (T, G))
    iv[rng.random((T, G)) < 0.1] = 0.0
    g64 = genes.astype(np.float64)
    bfrag = _dev(eng, rs.bfrag_encode(rows, N))
    D = [(g64 @ rows[t].astype(np.float64).T).astype(np.int64) for t in range(T)]   # exact: integers below 2^53
    dobs = np.stack([np.abs(D[t][np.arange(G), rng.integers(0, P, G)]) for t in range(T)])
    plain = _count_pass(eng, gm, bfrag, _dev(eng, dobs.astype(np.int32)), T, N, P)
    seen = set()
    for cc in (0, 1):
        # s_obs = the statistic of a random column of every gene: counts between 0 and P, ties where iv = 0
        sobs = np.stack([wy.stats(dobs[t], cc, iv[t]) for t in range(T)])
        order32, ss = eng.rank_stepdown_order(_dev(eng, sobs))
        order = order32.cpu().numpy()
        r_rank, c_rank, mx = _sd_pass(eng, gm, order, sobs, iv, dobs, bfrag, cc, N, P)
        assert (mx[:, P:] == SENTINEL).all()
        for t in (range(T) if cc else (0, T - 1)):                   # (cc = 0: the first and the last trait)
            ref = sd.stepdown(D[t], cc, iv[t], sobs[t])
            assert np.array_equal(order[t], ref["order"]), (cc, t)
            bad = np.flatnonzero(c_rank[t] != R0 + ref["c"])
            assert len(bad) == 0, "cc %d, trait %d: c differs at %d of %d ranks, first %s" % (cc, t, len(bad), G,
                                                                                             bad[:5].tolist())
            assert _same_bits(mx[t, :P], ref["u"][0]), (cc, t)
            assert np.array_equal(r_rank[t] - R0, plain[t][order[t]]), (cc, t)
            seen.update(np.unique(ref["c"]).tolist())
            del ref
    assert min(seen) < P // 2 and P in seen and len(seen) > 10


# ---------------------------------------------------------------- 3. tie groups ------
def test_tie_groups_across_runs_halves_groups_and_blocks(eng):
    """Duplicated gene rows put groups of equal s_obs across the ranks 0/1 (a copy of the top gene), 3/4 (two runs of
    four), 31/32 (the two row tiles), 62/63/64 (two groups of 64) and 255/256 (two blocks); the untestable genes sit
    at the tail.  The table is built in rank order -- every copy is the gene one rank ahead, which keeps the order --
    and then shuffled, so ss at rank k is the unshuffled table's s_obs[k] wherever the copies stand."""
    G, N, P = 300, 90, 130
    rng = np.random.default_rng(34)
    vals = (rng.permutation(N) * 1.0)[None]
    base = (rng.random((G, N)) < rng.uniform(0.2, 0.8, (G, 1))).astype(np.uint8)
    base[G - 2], base[G - 1] = 0, 1                                  # untestable: they sort last
    pre = _ranksum_reference(base, vals)
    ranked = base[sd.order_of(pre["s_obs"][0])]
    copies = (1, 4, 32, 63, 64, 256)
    for k in copies:
        ranked[k] = ranked[k - 1]
    want_ss = _ranksum_reference(ranked, vals)["s_obs"][0]
    assert (np.diff(want_ss) <= 0).all() and all(want_ss[k] == want_ss[k - 1] for k in copies)
    assert want_ss[61] > want_ss[62] == want_ss[64] > want_ss[65] and want_ss[-1] == 0.0 == want_ss[-2]
    genes = ranked[rng.permutation(G)]
    ref, sdref, r, rsd, rf = _check_ranksum_shape(eng, G, N, P, T=1, genes=genes, vals=vals)
    order, ss = sdref[0]["order"], sdref[0]["ss"]
    assert _same_bits(ss, want_ss) and not np.array_equal(order, np.arange(G))
    by_rank = rsd[0][order]
    for k in copies:
        assert by_rank[k] == by_rank[k - 1], k
    assert (by_rank[-2:] == P).all() and (np.diff(by_rank) >= 0).all() and by_rank[0] == rf[0][order[0]]
    assert (r <= rsd).all() and (rsd <= rf).all()


# ---------------------------------------------------------------- 4. traits that cannot be tested ------
def test_untestable_traits_have_zero_maxima_and_r_sd_p(eng):
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
    r, rf, rsd, mx = (x.cpu().numpy() for x in eng.ranksum_stepdown(gm, plan, res, P, SEED))
    wr, wrf, wmx = (x.cpu().numpy() for x in eng.ranksum_westfall_young(gm, plan, res, P, SEED))
    assert np.array_equal(r, wr) and np.array_equal(rf, wrf) and _same_bits(mx, wmx)
    assert mx.shape == (3, P) and not mx[0].any() and not mx[2].any() and (mx[1] > 0).all()
    assert (rsd[0] == P).all() and (rsd[2] == P).all()
    ref = _ranksum_reference(genes, vals)
    D = _products(genes, eng.ranksum_values(plan, 0, P, SEED).cpu().numpy())
    assert np.array_equal(rsd[1], sd.stepdown(D[1], 1, ref["iv"][1], ref["s_obs"][1])["r_sd"])
    assert (r <= rsd).all() and (rsd <= rf).all() and (rsd[1, [1, 2]] == P).all()


# ---------------------------------------------------------------- 5. where the maximum sits ------
def test_a_maximum_in_the_last_group_only_and_one_in_the_first_row(eng):
    """G = 513: nine groups in three blocks.  Trait 0: only the gene at the last rank (alone in group 8) has iv > 0,
    so every u[k] of a column is that gene's s: the suffix crosses every group and block boundary.  Trait 1: only
    the gene at rank 0 has iv > 0: u[0] = its s and u[k] = 0 behind it."""
    G, N, P, T = 513, 33, 65, 2
    rng = np.random.default_rng(513)
    genes = (rng.random((G, N)) < 0.5).astype(np.uint8)
    rows = rng.integers(-200, 201, (T, P, N))
    D = _products(genes, rows)
    sobs = np.sort(rng.uniform(1.0, 2.0, (T, G)), axis=1)[:, ::-1].copy()
    perm = rng.permutation(G)
    sobs = sobs[:, perm]                                             # rank k is gene order[k], not gene k
    order = np.stack([sd.order_of(sobs[t]) for t in range(T)])
    iv = np.zeros((T, G))
    last, first = order[0, G - 1], order[1, 0]
    # a scale that puts s among the s_obs: some columns count, some do not
    iv[0, last] = 1.5 / np.median(np.abs(D[0, last]).astype(np.float64) ** 2 + 1.0)
    iv[1, first] = 1.5 / np.median(np.abs(D[1, first]).astype(np.float64) ** 2 + 1.0)
    dobs = np.abs(D[:, :, 3])
    bfrag = _dev(eng, rs.bfrag_encode(rows, N))
    for cc in (0, 1):
        ref, _r, _rsd, _rf = _check_against_spec(eng, genes, D, dobs, iv, sobs, bfrag, cc, N, P, ("planted", cc))
        assert (ref[0]["u"] == ref[0]["u"][G - 1]).all() and ref[0]["u"][G - 1].max() > 1.0
        assert not ref[1]["u"][1:].any() and ref[1]["u"][0].max() > 1.0
        assert len(np.unique(ref[0]["c"])) > 3 and ref[1]["c"][1:].max() == 0 and ref[1]["c"][0] > 0


# ---------------------------------------------------------------- 6. batches ------
def test_two_batches_of_64_are_one_of_128(eng):
    G, N, P, T = 300, 257, 128, 2
    rng = np.random.default_rng(128)
    genes, vals = _genes(rng, G, N), _values(rng, T, N)
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(vals)
    res = eng.ranksum(gm, plan)
    assert eng.rank_stepdown_batch(G, T, N, P, 1) == 64 and eng.rank_stepdown_batch(G, T, N, P) == 128
    one = [x.cpu().numpy() for x in eng.ranksum_stepdown(gm, plan, res, P, SEED)]
    two = [x.cpu().numpy() for x in eng.ranksum_stepdown(gm, plan, res, P, SEED, budget_bytes=1)]
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    ref = _ranksum_reference(genes, vals)
    D = _products(genes, eng.ranksum_values(plan, 0, P, SEED).cpu().numpy())
    for t in range(T):
        want = sd.stepdown(D[t], 1, ref["iv"][t], ref["s_obs"][t])
        assert np.array_equal(one[2][t], want["r_sd"]) and _same_bits(one[3][t], want["u"][0])
        assert np.array_equal(one[0][t], wy.r_count(D[t], ref["d"][t]))
        assert np.array_equal(one[1][t], wy.r_fwer(one[3][t], ref["s_obs"][t]))
    wy_run = [x.cpu().numpy() for x in eng.ranksum_westfall_young(gm, plan, res, P, SEED)]
    assert np.array_equal(one[0], wy_run[0]) and np.array_equal(one[1], wy_run[1]) and _same_bits(one[3], wy_run[2])
    # the second batch alone through the raw entry point: perm_base = 64 writes the columns 64 .. 127 of maxs
    order32, _ss = eng.rank_stepdown_order(_dev(eng, ref["s_obs"]))
    r_rank, c_rank, mx = _sd_pass(eng, gm, order32.cpu().numpy(), ref["s_obs"], ref["iv"], ref["d"],
                                  _ranksum_bfrag(eng, plan, 64, perm_base=64), 1, N, 64, before=64)
    assert (mx[:, :64] == SENTINEL).all() and (mx[:, 128:] == SENTINEL).all() and _same_bits(mx[:, 64:128], one[3][:, 64:])
    for t in range(T):
        assert np.array_equal(c_rank[t] - R0, sd.stepdown(D[t][:, 64:], 1, ref["iv"][t], ref["s_obs"][t])["c"])


# ---------------------------------------------------------------- 7. S16 ------
def test_van_elteren_nine_strata(eng):
    """S = 9 at N = 333, strata of uneven size with one of a single isolate and one of two; P = 130 in batches of 64."""
    G, N, P, T, S = 150, 333, 130, 2, 9
    rng = np.random.default_rng(333)
    genes, vals = _genes(rng, G, N), _values(rng, T, N)
    st = rng.integers(0, S - 2, N)
    st[5], st[[50, 60]] = S - 2, S - 1
    vals[:, [5, 50, 60]] = [[1.0, 2.0, 3.0]]
    gm = eng.pack_dense(genes)
    plan = eng.vanelteren_plan(vals, st)
    res = eng.vanelteren(gm, plan)
    r, rf, rsd, mx = (x.cpu().numpy() for x in eng.vanelteren_stepdown(gm, plan, res, P, SEED, budget_bytes=1))
    wr, wrf, wmx = (x.cpu().numpy() for x in eng.vanelteren_westfall_young(gm, plan, res, P, SEED))
    assert np.array_equal(r, wr) and np.array_equal(rf, wrf) and _same_bits(mx, wmx)
    assert np.array_equal(r, eng.vanelteren_permute(gm, plan, res["d"], P, SEED).cpu().numpy())
    D = _products(genes, eng.vanelteren_values(plan, 0, P, SEED).cpu().numpy())
    for t in range(T):
        pr = wy.vanelteren_problem(genes.tolist(), [float(v) for v in vals[t]], [int(s) for s in st], S)
        want = sd.stepdown(D[t], 0, pr["iv"], pr["s_obs"])
        assert np.array_equal(rsd[t], want["r_sd"]) and _same_bits(mx[t], want["u"][0]), t
        assert (rsd[t][np.asarray(pr["iv"]) == 0] == P).all()
    assert (r <= rsd).all() and (rsd <= rf).all() and (rsd > r).any()


# ---------------------------------------------------------------- 8. the planted driver of the host test ------
def test_the_planted_driver_is_not_the_single_step_count(eng):
    genes, values, pr, D, out, r, rf = sd.planted_problem()
    assert (out["r_sd"] < rf).any()                                   # (the host test's assertion, once more)
    P = sd.PLANTED_P
    gm = eng.pack_dense(genes)
    plan = eng.ranksum_plan(values[None])
    res = eng.ranksum(gm, plan)
    got = [x.cpu().numpy() for x in eng.ranksum_stepdown(gm, plan, res, P, sd.PLANTED_SEED)]
    assert np.array_equal(_products(genes, eng.ranksum_values(plan, 0, P, sd.PLANTED_SEED).cpu().numpy())[0], D)
    assert np.array_equal(got[0][0], r) and np.array_equal(got[1][0], rf) and np.array_equal(got[2][0], out["r_sd"])
    assert _same_bits(got[3][0], out["u"][0]) and (got[2][0] < got[1][0]).any()


# ---------------------------------------------------------------- 9. arguments and resources ------
def test_argument_checks(eng):
    import torch
    G, N, P, T = 4, 40, 3, 1
    gm = eng.pack_dense(np.ones((G, N), dtype=np.uint8))
    need = int(eng.lib.scoary_rank_stepdown_scratch_bytes(eng.h, G, T, N, P))
    gp, qp = eng.padded_genes(G), int(eng.lib.scoary_tiled_quads(N))
    assert need == T * (qp * gp * 16 + gp * 20 + (gp // 64) * 64 * 8)
    assert eng.lib.scoary_rank_stepdown_scratch_bytes(eng.h, 0, T, N, P) == 0
    assert int(eng.lib.scoary_rank_stepdown_scratch_bytes(eng.h, G, T, N, 65)) - need == T * (gp // 64) * 64 * 8
    z = torch.zeros((T, 64), dtype=torch.float64, device=eng.device)
    d = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    o = torch.arange(G, dtype=torch.int32, device=eng.device).reshape(T, G).contiguous()
    r = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    c = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    b = torch.zeros((int(eng.lib.scoary_ranksum_bfrag_bytes(N, P, T)),), dtype=torch.uint8, device=eng.device)
    scratch = torch.zeros((need,), dtype=torch.uint8, device=eng.device)

    def gather(n=N, t=T):
        return eng.lib.scoary_rank_stepdown_gather(eng.h, eng._ptr(gm.tiled), eng._ptr(o), eng._ptr(z), eng._ptr(z),
                                                   eng._ptr(d), G, t, n, eng._ptr(scratch), eng._stream())

    def call(cc=1, n=N, p=P, stride=P, t=T, base=0):
        return eng.lib.scoary_permute_rank_stepdown(eng.h, eng._ptr(scratch), eng._ptr(b), cc, G, t, n, p, base,
                                                    eng._ptr(r), eng._ptr(c), eng._ptr(z), stride, eng._stream())
    for kw in (dict(cc=2), dict(cc=-1), dict(stride=P - 1), dict(p=0), dict(base=-1), dict(base=1)):
        assert call(**kw) == ERR_ARG, kw
    for kw in (dict(n=rs.MAX_ISOLATES + 1), dict(t=65536), dict(p=1 << 31, stride=1 << 31)):
        assert call(**kw) == ERR_SIZE, kw
    assert gather(n=rs.MAX_ISOLATES + 1) == ERR_SIZE and gather(t=65536) == ERR_SIZE and gather(n=0) == ERR_ARG
    torch.cuda.synchronize()
    assert not r.any().item() and not c.any().item() and not z.any().item() and not scratch.any().item()
    assert gather() == 0 and call() == 0        # thresholds 0, iv 0, ss 0: every column counts, every maximum is 0
    torch.cuda.synchronize()
    assert (r == P).all().item() and (c == P).all().item() and not z.any().item()
    # an entry of the order that is no gene makes a padded position: zero row, iv 0, a threshold nothing reaches
    o[0, 1], o[0, 2] = G + 5, -1
    r.zero_()
    c.zero_()
    assert gather() == 0 and call() == 0
    torch.cuda.synchronize()
    assert r[0].tolist() == [P, 0, 0, P] and (c == P).all().item() and not z.any().item()


def test_resource_rules_and_the_kernels_that_were_there():
    import json
    import __graft_entry__ as ge
    with open(ge.HIP_RESOURCES) as f:
        res = json.load(f)
    ge.check_kernel_resources(res, ge.RANK_SD_RULES)
    ge.check_kernel_resources(res, ge.RANK_WY_RULES + ge.RANKSUM_RULES)
    # the resource lines of the kernels the new file restates, as the compiler reported them before it existed
    was = {"k_rank_maxt": {"VGPRs": 240, "AGPRs": 0, "SGPRs Spill": 0, "VGPRs Spill": 0, "ScratchSize": 0,
                           "TotalSGPRs": 63, "Occupancy": 2, "LDS Size": 0},
           "k_permute_ranksum": {"VGPRs": 237, "AGPRs": 0, "SGPRs Spill": 2, "VGPRs Spill": 0, "ScratchSize": 0,
                                 "TotalSGPRs": 106, "Occupancy": 2, "LDS Size": 0}}
    for name, want in was.items():
        (got,) = [v for k, v in res.items() if name in k]
        assert {k: got[k] for k in want} == want, name
    for name in ("k_rank_sd_max", "k_rank_sd_count"):
        (got,) = [v for k, v in res.items() if name in k]
        assert got["Occupancy"] == 2 and got["VGPRs"] + got["AGPRs"] <= 256 and got["ScratchSize"] == 0
