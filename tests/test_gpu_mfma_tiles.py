"""k_permute_mfma on 16x16x128 tiles: the lane maps of its operands, accumulators and thresholds.

The kernel reads the A panels and the B fragments in 16-byte pieces (32 isolates of one slot, or of one
permutation) and puts them together as fragments of v_mfma_f32_16x16x128_f8f6f4: lane l of a fragment holds
row (column) l & 15, isolates 32 (l >> 4) .. + 31 of a K-step of 128; lane l of an accumulator tile holds column
l & 15, rows 4 (l >> 4) + r.  A wavefront's 32 slots are two row tiles, a stage's 64 permutations four column
tiles.  A wrong piece address, group order, row or column map changes counts, so exact equality of r with a path
that shares none of this is the whole check:

  steps     engine.associate with every slot routed against the dense AND+popcount kernel (use_lists=False), on
            every (trait, gene) pair
  regions   scoary_permute_hybrid under intervals chosen here against the oracle's labels x a float64 matrix
            product (tests/probe_regions.py)

Shapes: G = 20 (one partly filled wavefront), 272 (a second block with one 16-row tile), 300 (a ragged second
block: rows end inside a tile, at no multiple of 4); N = 31, 100, 129 (a second K-step with one group of 32),
2000, 2048; P = 1, 16, 17, 64, 65, 200 (a ragged column tile, a ragged stage, several stages).
"""
import ctypes

import numpy as np
import pytest

import probe_regions as pr

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.set_mfma_route("auto")
    e.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cache():
    """Problems shared by the tests of this module (built once, never changed)."""
    c = {}
    yield c
    c.clear()


class Problem:
    pass


def _traits(N, T, seed):
    """Trait 1 (and 2) with missing values, in different places."""
    rng = np.random.default_rng(seed)
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    if T > 1:
        traits[1, ::29] = 2
    if T > 2:
        traits[2, 5::17] = 2
    return traits


def _problem(eng, cache, G, N, T=3, seed=41):
    """Genes over the whole frequency range (above 0.5: flipped lists), an absent and a core gene."""
    key = (G, N, T)
    if key in cache:
        return cache[key]
    from scoary_amd.engine import pack_bits_rows
    rng = np.random.default_rng(seed)
    p = Problem()
    p.G, p.N, p.T = G, N, T
    p.genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    p.genes[3] = 0
    p.genes[4] = 1
    p.traits = _traits(N, T, seed + 1)
    p.tb = pack_bits_rows((p.traits == 1).astype(np.uint8))
    p.mb = pack_bits_rows((p.traits != 2).astype(np.uint8))
    p.gm = eng.pack_dense(p.genes)
    eng.build_lists(p.gm)
    assert p.gm.lists.panels is not None
    p.trv, p.mkv = eng.vecrows(p.tb, N), eng.vecrows(p.mb, N)
    cache[key] = p
    return p


def _dense(eng, p, P, seed):
    res = eng.associate(p.gm, p.trv, p.mkv, permutations=P, seed=seed, use_lists=False)
    return res["r"].cpu().numpy().view(np.uint32).copy()


def _routed(eng, p, P, seed, split=None):
    """One step through the list path with every slot on the matrix cores (split: the first `split` slots)."""
    eng.set_mfma_route("all")
    try:
        assert eng.mfma_split(p.gm, p.T, P) == (p.G if split is None else split)
        res = eng.associate(p.gm, p.trv, p.mkv, permutations=P, seed=seed, use_lists=True, graph=False)
        return res["r"].cpu().numpy().view(np.uint32).copy()
    finally:
        eng.set_mfma_route("auto")


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d of %d pairs differ from the reference, first (trait, gene, got, want) %s" % (
        what, len(bad), want.size, [(int(t), int(g), int(got[t, g]), int(want[t, g])) for t, g in bad[:6]])


# ------------------------------------------------------------------ rows x K ------
@pytest.mark.parametrize("N", [31, 100, 129, 2000, 2048])
@pytest.mark.parametrize("G", [20, 272, 300])
def test_rows_and_k_steps(eng, cache, G, N):
    """Both row tiles and the end of the rows at and off a 4-row boundary, against every K-step count from one group
    of 31 isolates to all sixteen K-steps; P = 130 is two whole stages and a ragged one of two columns."""
    p = _problem(eng, cache, G, N)
    P, seed = 130, 7
    _same(_routed(eng, p, P, seed), _dense(eng, p, P, seed), "G=%d N=%d" % (G, N))


# ------------------------------------------------------------------ columns ------
@pytest.mark.parametrize("P", [1, 16, 17, 64, 65, 200])
def test_columns(eng, cache, P):
    """One column, one whole column tile, one column into the second tile, one whole stage, one column into the
    second stage, four stages with a last one of eight columns."""
    p = _problem(eng, cache, 300, 129)
    _same(_routed(eng, p, P, 100 + P), _dense(eng, p, P, 100 + P), "P=%d" % P)


# ------------------------------------------------------------------ trait switches inside a range ------
def test_one_range_spans_the_traits(eng, cache):
    """T = 3, P = 130: three stages per trait and one partial tile, so ranges are cut on trait boundaries only, and
    with more gene blocks than a round over the CUs can take three times the launch is one range of nine stages per
    block: two segments end inside the loop (ragged last stage, lane reduction, store, the next trait's centres as
    C), one behind it.  Traits 1 and 2 have missing values."""
    import torch
    G, N, T, P = 43_800, 100, 3, 130
    out = (ctypes.c_int64 * 4)()
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert eng.lib.scoary_mfma_plan(num_cu, G, T, P, out) == 0
    assert (int(out[1]), int(out[2])) == (1, 9), "plan (ranges, L) = %s: not one range over the three traits" % (
        [int(v) for v in out],)
    p = _problem(eng, cache, G, N, T)
    _same(_routed(eng, p, P, 5), _dense(eng, p, P, 5), "one range, three traits")


# ------------------------------------------------------------------ chosen regions ------
def _regions_problem(eng, orc, cache):
    key = "regions"
    if key in cache:
        return cache[key]
    G, N, T, P, seed = 300, 129, 3, 81, 19
    p = _problem(eng, cache, G, N, T)
    q = Problem()
    q.p, q.P = p, P
    q.counts, q.margins = eng.counts(p.gm, p.trv, p.mkv)
    q.npos = (p.traits == 1).sum(1).astype(np.int64)
    flipped = pr.flip_rule(p.genes)
    assert np.array_equal(p.gm.lists.flipped.cpu().numpy().astype(bool), flipped)
    minority = pr.minority_rows(p.genes, flipped)
    L = minority.sum(1, dtype=np.int64)
    q.order = p.gm.lists.order.cpu().numpy().astype(np.int64)
    pr.check_order(q.order, L)
    q.m = pr.slot_limits(L, q.npos, q.order)
    q.tiles = eng.perm_generate_tiles(p.mkv, q.margins, N, P, 0, seed)
    q.u = pr.overlap_counts(minority, pr.oracle_labels(orc, seed, p.traits, P))
    assert np.all(q.u[:, q.order, :].max(-1) <= q.m)
    cache[key] = q
    return q


def _region_r(eng, q, lo, hi1):
    """One scoary_permute_hybrid launch, every slot routed: poisoned scratch and fragments, sentinel r."""
    import torch
    p = q.p
    scratch = eng.permute_lists_scratch(p.G, p.T, p.N, q.P)
    scratch.fill_(-1)
    words = int(eng.lib.scoary_mfma_bfrag_bytes(p.N, q.P, p.T)) // 4
    bfrag = torch.full((words,), -1, dtype=torch.int32, device=eng.device)
    r = torch.full((p.T, p.G), SENTINEL, dtype=torch.int32, device=eng.device)
    lc = torch.from_numpy(np.ascontiguousarray(np.stack([lo, hi1], axis=-1), dtype=np.int32)).to(eng.device)
    eng.set_mfma_route("all")
    try:
        assert eng.mfma_split(p.gm, p.T, q.P) == p.G
        eng.permute_lists(p.gm, q.tiles, None, q.margins, q.P, r, scratch=scratch, lcrit=lc, accumulate=False,
                          bfrag=bfrag)
    finally:
        eng.set_mfma_route("auto")
    return r.cpu().numpy().view(np.uint32).copy()


def test_edge_and_random_regions(eng, orc, cache):
    """(0, 0): the span-0 region, r = P; [0, m + 1): r = 0; the intervals next to either end of the support; two
    random interval arrays."""
    q = _regions_problem(eng, orc, cache)
    fams = [(name, lo, hi1) for name, (lo, hi1) in pr.edge_regions(q.m).items()]
    fams += [("random seed %d" % s,) + pr.random_regions(q.m, s) for s in (1, 2)]
    for name, lo, hi1 in fams:
        lo, hi1 = pr.check_regions(lo, hi1, q.m)
        got = _region_r(eng, q, lo, hi1)
        _same(got, pr.r_ref(q.u, q.order, lo, hi1), name)
        if name == "(0,0)":
            assert np.all(got == q.P)
        if name == "[0,m+1)":
            assert not got.any()


def test_point_regions_around_every_count(eng, orc, cache):
    """The point intervals [v, v + 1) over every value u takes and one on either side: with u at lo - 1, lo = hi1 - 1
    and hi1 the centre taken as C and the half-width compare decide each permutation on its own; the hits of a pair
    over its distinct v are all P permutations."""
    q = _regions_problem(eng, orc, cache)
    us = q.u[:, q.order, :]
    total = np.zeros((q.p.T, q.p.G), dtype=np.int64)
    prev = None
    for j, v in enumerate(pr.sweep_launches(q.u, q.order, q.m)):
        lo, hi1 = pr.check_regions(v, v + 1, q.m)
        got = _region_r(eng, q, lo, hi1)
        _same(got, pr.r_ref(q.u, q.order, lo, hi1), "point intervals, launch %d" % j)
        hits = q.P - got[:, q.order].astype(np.int64)
        assert np.array_equal(hits, (us == v[..., None]).sum(-1))
        total += np.where(True if prev is None else v != prev, hits, 0)      # v only grows: repeats are neighbours
        prev = v
    assert np.all(total == q.P)


# ------------------------------------------------------------------ split ------
def test_forced_split_at_256_slots(eng, cache, monkeypatch):
    """Slots [0, 256) on the matrix cores, [256, 600) on the list walk: both kernels write one `partial`."""
    p = _problem(eng, cache, 600, 129)
    P, seed = 200, 3
    want = _dense(eng, p, P, seed)
    monkeypatch.setattr(eng, "mfma_split", lambda genes, T, P: 256)
    _same(_routed(eng, p, P, seed, split=256), want, "split at 256 of 600 slots")


# ------------------------------------------------------------------ graph replay ------
def test_captured_step_replays(eng, cache):
    import torch
    p = _problem(eng, cache, 300, 129)
    P, seed = 200, 3
    want = _dense(eng, p, P, seed)
    eng.set_mfma_route("all")
    try:
        ws = eng.workspace(p.gm, p.T, P, use_lists=True)
        plan = eng.trait_plan(p.trv, p.mkv, p.N)
        graph, res = eng.capture(p.gm, p.trv, p.mkv, P, seed, ws, use_lists=True, plan=plan)
        res["r"].zero_()
        graph.launch()
        torch.cuda.synchronize()
        got = res["r"].cpu().numpy().view(np.uint32).copy()
        graph.close()
    finally:
        eng.set_mfma_route("auto")
    _same(got, want, "captured step, one replay")
