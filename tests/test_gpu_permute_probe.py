"""The permutation kernels' exact overlap counts, read out through synthetic rejection regions.

r[t][g] = #{pi : u < lo or u >= hi1}: the acceptance interval [lo, hi1) of the list count u is an input of
scoary_permute_hybrid (slot order) and of scoary_permute (gene order), so a test that chooses it sees u
itself, not the two mid-distribution thresholds Fisher derives from the data.  Every case below compares r
on EVERY (trait, gene) pair with a numpy reference that shares no code with the kernels
(tests/probe_regions.py: the oracle's labels, a float64 matrix product, a compare):

  edges    (0, 0) -> r = P, [0, m + 1) -> r = 0, [0, 1), [m, m + 1), [1, m + 1), [0, m); m = min(L, npos)
  random   (lo, hi1) independent per (trait, slot), uniform on 0 <= lo <= hi1 <= m + 1, two seeds
  sweep    the point intervals [v, v + 1) over every value u takes and one beside: r = P - #{u = v}, and
           the hits of one pair over its distinct v sum to P -- the whole histogram of u

on matrices whose first rows are an absent and a core gene, one-hot genes (isolates 0, 1, 31, 32, 63, 64,
1023, 1024, 2046, 2047, N - 1; their u is one label bit) and their complements, genes at the flip tie and
one carried by the isolates missing in trait 1; traits with two sets of missing values, one positive, and
all but one positive.  All intervals lie in 0 <= lo <= hi1 <= min(L, npos) + 1, inside the domain
k_lists_crit documents (hi1 <= npos + 1 <= N + 1 < 2^(KC+1)): nothing had to be clamped.

The A panels of the matrix-core kernel are also decoded and compared with the minority rows directly: ones
beyond isolate N in a panel meet label rows that k_mfma_bfrag zeroes too, so no r can show them.

Every permute_lists call gets a scratch tensor and a B-fragment buffer filled with 0xFF bytes and, without
accumulate, an r filled with a sentinel: a partial count that no kernel writes cannot pass as last launch's.

The matrix-core path's zero fill of the partial tiles beyond its ranges: scoary_mfma_geom makes one range
per partial tile whenever the blocks fit one round over the CUs (P = 1100: three tiles, three ranges, no
tile left to zero), so next to that case one with more tiles than the 64 ranges a trait can have
(P = 33 000: 65 tiles, 516 stages, 9 per range, 58 ranges -- tiles 58 .. 64 hold zeros only) and the
16-bit cases (P = 65 472: one range, 127 zero tiles) put it on the line.

16-bit range count: one k_permute_mfma range counts at most 1023 stages x 64 = 65 472 permutations in a
uint16_t.  P = 65 472 / 65 473 / 70 000 at 256 blocks (one round over 256 CUs: the geometry has no reason to
cut ranges short) run in ONE call each -- the C ABI takes them -- under (0, 0) (every range counts all its
permutations), [0, m + 1) and one random interval array, the latter against the dense kernel.

Which of these tests turn red under which one-line mutation of the kernels, next to the existing stagger and
hybrid files: profiles/r12_permute_probe.txt.
"""
import contextlib

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
    """Problems and label sets shared by the tests of this module (built once, never changed)."""
    c = {}
    yield c
    c.clear()


class Problem:
    pass


class Labels:
    pass


def _problem(eng, cache, key, genes, traits):
    """Everything of a (gene matrix, traits) pair: device matrix + lists, and on the host the flip rule, the
    minority rows, the slot order (checked against the device's) and m = min(L, npos) per (trait, slot)."""
    if key in cache:
        return cache[key]
    from scoary_amd.engine import pack_bits_rows
    p = Problem()
    p.genes, p.traits = genes, traits
    p.G, p.N = genes.shape
    p.T = traits.shape[0]
    tb = pack_bits_rows((traits == 1).astype(np.uint8))
    mb = pack_bits_rows((traits != 2).astype(np.uint8))
    p.gm = eng.pack_dense(genes)
    eng.build_lists(p.gm)
    p.trv, p.mkv = eng.vecrows(tb, p.N), eng.vecrows(mb, p.N)
    p.counts, p.margins = eng.counts(p.gm, p.trv, p.mkv)
    p.npos = (traits == 1).sum(1).astype(np.int64)
    nval = (traits != 2).sum(1).astype(np.int64)
    assert np.array_equal(p.margins.cpu().numpy(), np.stack([p.npos, nval], axis=1))
    p.flipped = pr.flip_rule(genes)
    assert np.array_equal(p.gm.lists.flipped.cpu().numpy().astype(bool), p.flipped)
    p.minority = pr.minority_rows(genes, p.flipped)
    p.L = p.minority.sum(1, dtype=np.int64)
    p.order = p.gm.lists.order.cpu().numpy().astype(np.int64)
    pr.check_order(p.order, p.L)
    p.m = pr.slot_limits(p.L, p.npos, p.order)
    cache[key] = p
    return p


def _probe_problem(eng, cache, G, N, T=5, with_empty=True, extra_hots=()):
    key = ("probe", G, N, T, with_empty)
    if key in cache:
        return cache[key]
    traits = pr.probe_traits(N, 23, T)
    genes, _names = pr.probe_genes(G, N, traits, 23, extra_hots=extra_hots, with_empty=with_empty)
    return _problem(eng, cache, key, genes, traits)


def _labels(eng, orc, cache, prob_key, p, P, rows=False):
    """Label tiles (and, for the dense kernel, label rows) of P permutations, generated once, and the
    reference's u from the oracle's labels of the same seed."""
    key = ("labels", prob_key, P)
    lb = cache.get(key)
    if lb is None:
        lb = Labels()
        lb.P, lb.seed = P, 100 + P
        lb.tiles = eng.perm_generate_tiles(p.mkv, p.margins, p.N, P, 0, lb.seed)
        lb.rows = None
        lb.u = pr.overlap_counts(p.minority, pr.oracle_labels(orc, lb.seed, p.traits, P))
        assert np.all(lb.u[:, p.order, :].max(-1) <= p.m)
        cache[key] = lb
    if rows and lb.rows is None:
        lb.rows = eng.perm_generate(p.mkv, p.margins, p.N, P, 0, lb.seed)
    return lb


@contextlib.contextmanager
def _route(eng, mode, p, P):
    """Routing "all" (every slot on the matrix cores) or "none" (every slot on the list walk)."""
    eng.set_mfma_route(mode)
    try:
        assert eng.mfma_split(p.gm, p.T, P) == (p.G if mode == "all" else 0)
        yield
    finally:
        eng.set_mfma_route("auto")


def _poisoned(eng, p, P):
    import torch
    scratch = eng.permute_lists_scratch(p.G, p.T, p.N, P)
    scratch.fill_(-1)
    bfrag = None
    if p.gm.lists.panels is not None:
        words = int(eng.lib.scoary_mfma_bfrag_bytes(p.N, P, p.T)) // 4
        bfrag = torch.full((words,), -1, dtype=torch.int32, device=eng.device)
    return scratch, bfrag


def _lists_r(eng, p, tiles, P, lo=None, hi1=None, crit=None, r=None, accumulate=False):
    """One scoary_permute_hybrid launch under the current routing: slot-order intervals (lo, hi1), or
    gene-order ``crit`` through k_lists_crit; poisoned scratch, sentinel r."""
    import torch
    scratch, bfrag = _poisoned(eng, p, P)
    if r is None:
        assert not accumulate
        r = torch.full((p.T, p.G), SENTINEL, dtype=torch.int32, device=eng.device)
    lc = cr = None
    if crit is not None:
        cr = torch.from_numpy(np.ascontiguousarray(crit, dtype=np.int32)).to(eng.device)
    else:
        lc = torch.from_numpy(np.ascontiguousarray(np.stack([lo, hi1], axis=-1), dtype=np.int32)).to(eng.device)
    eng.permute_lists(p.gm, tiles, cr, p.margins, P, r, scratch=scratch, lcrit=lc, accumulate=accumulate,
                      bfrag=bfrag)
    return r


def _host(r):
    return r.cpu().numpy().view(np.uint32).copy()


def _where(p, got, want, lo, hi1, what):
    """Which (trait, slot) pairs differ: the evidence a red case is located from."""
    slot_of = np.empty(p.G, dtype=np.int64)
    slot_of[p.order] = np.arange(p.G)
    bad = np.argwhere(got != want)
    lines = ["%s: %d of %d pairs differ (G=%d N=%d); first ones:" % (what, len(bad), want.size, p.G, p.N)]
    for t, g in bad[:12]:
        k = slot_of[g]
        lines.append("  t=%d gene=%d slot=%d L=%d flipped=%d [lo,hi1)=[%d,%d) got=%d want=%d"
                     % (t, g, k, p.L[g], p.flipped[g], lo[t, k], hi1[t, k], got[t, g], want[t, g]))
    return "\n".join(lines)


def _expect(eng, p, lb, lo, hi1, what, crit=False, factor=1, **kw):
    lo, hi1 = pr.check_regions(lo, hi1, p.m)
    want = factor * pr.r_ref(lb.u, p.order, lo, hi1)
    c = pr.gene_order_crit(lo, hi1, p.order, p.flipped, p.npos) if crit else None
    r = _lists_r(eng, p, lb.tiles, lb.P, lo, hi1, crit=c, **kw)
    got = _host(r)
    assert np.array_equal(got, want), _where(p, got, want, lo, hi1, what)
    return r, got


def _families(p):
    fams = [(name, lo, hi1) for name, (lo, hi1) in pr.edge_regions(p.m).items()]
    fams += [("random seed %d" % s,) + pr.random_regions(p.m, s) for s in (1, 2)]
    return fams


def _edges_and_random(eng, p, lb, tag, crit=False):
    for name, lo, hi1 in _families(p):
        _r, got = _expect(eng, p, lb, lo, hi1, "%s P=%d %s" % (tag, lb.P, name), crit=crit)
        if name == "(0,0)":
            assert np.all(got == lb.P)
        if name == "[0,m+1)":
            assert not got.any()


def _sweep(eng, p, lb, tag):
    """[v, v + 1) over every value of u: r = P - #{u = v} per launch, the hits of a pair sum to P."""
    vs = pr.sweep_launches(lb.u, p.order, p.m)
    us = lb.u[:, p.order, :]
    total = np.zeros((p.T, p.G), dtype=np.int64)
    prev = None
    for j, v in enumerate(vs):
        _r, got = _expect(eng, p, lb, v, v + 1, "%s P=%d sweep launch %d of %d" % (tag, lb.P, j, len(vs)))
        hits = lb.P - got[:, p.order].astype(np.int64)
        assert np.array_equal(hits, (us == v[..., None]).sum(-1))
        total += np.where(True if prev is None else v != prev, hits, 0)      # v only grows: repeats are neighbours
        prev = v
    assert np.all(total == lb.P)
    return len(vs)


# ------------------------------------------------------------------ 1. k_permute_mfma ------
@pytest.mark.parametrize("N", [64, 65, 1000, 2048])
@pytest.mark.parametrize("G", [33, 300, 513])
def test_mfma_edges_and_random(eng, orc, cache, G, N):
    p = _probe_problem(eng, cache, G, N)
    assert p.gm.lists.panels is not None
    for P in (1, 65, 193):
        lb = _labels(eng, orc, cache, (G, N), p, P)
        with _route(eng, "all", p, P):
            _edges_and_random(eng, p, lb, "mfma")


@pytest.mark.parametrize("N", [64, 65, 1000, 2048])
@pytest.mark.parametrize("G", [33, 513])
def test_mfma_panels_hold_the_minority_rows(eng, cache, G, N):
    """The A operand itself, decoded by the layout scoary_mfma.hip documents: [wave panel of 64 slots][row tile]
    [K-step][lane] x 16 bytes, lane l = slot 32 i + (l & 31) of the panel, isolates 64 k + 32 (l >> 5) .. + 31,
    one E2M1 nibble per isolate (0 or 0x2 = 1.0).  Isolates >= N and slots >= G are zero: k_mfma_bfrag
    zeroes the label rows >= N as well, so r alone does not show a panel that carries ones there."""
    p = _probe_problem(eng, cache, G, N)
    by = p.gm.lists.panels.cpu().numpy().view(np.uint8)
    Gp = -(-G // 256) * 256
    assert by.size == Gp * 1024
    by = by.reshape(Gp // 64, 2, 32, 2, 32, 16)          # panel, row tile, K-step, isolate half, slot, byte
    nib = np.stack([by & 15, by >> 4], axis=-1)          # byte b: isolates 2 b (low nibble) and 2 b + 1
    assert np.isin(nib, (0, 2)).all()
    rows = (nib == 2).reshape(Gp // 64, 2, 32, 2, 32, 32).transpose(0, 1, 4, 2, 3, 5).reshape(Gp, 2048)
    want = np.zeros((Gp, 2048), dtype=bool)
    want[:G, :N] = p.minority[p.order].astype(bool)
    bad = np.argwhere(rows != want)
    assert not len(bad), "%d panel entries differ; first (slot, isolate): %s" % (len(bad), bad[:8].tolist())


@pytest.mark.parametrize("G,N,P", [(300, 65, 129), (513, 1000, 193), (33, 2048, 1100)])
def test_mfma_sweep(eng, orc, cache, G, N, P):
    p = _probe_problem(eng, cache, G, N)
    lb = _labels(eng, orc, cache, (G, N), p, P)
    with _route(eng, "all", p, P):
        J = _sweep(eng, p, lb, "mfma")
    print("sweep G=%d N=%d P=%d: J = %d launches" % (G, N, P, J))


@pytest.mark.parametrize("N,mode", [(256, "all"), (256, "none"), (2048, "all")])
def test_identity_matrix_reads_every_isolate_once(eng, orc, cache, N, mode):
    """The N x N identity and its complement: the u of slot k is the label bit of one isolate."""
    key = ("identity", N)
    p = cache.get(key) or _problem(eng, cache, key, pr.identity_genes(N), pr.probe_traits(N, 29))
    assert np.all(p.L == 1) and p.flipped[N:].all() and not p.flipped[:N].any()
    P = 65
    lb = _labels(eng, orc, cache, key, p, P)
    with _route(eng, mode, p, P):
        _edges_and_random(eng, p, lb, "identity %s" % mode)


# ------------------------------------------------------------------ 2. k_permute_lists, TW = 16 ------
@pytest.mark.parametrize("G,N,P", [(300, 65, 129), (513, 1000, 193)])
def test_lists_edges_and_random(eng, orc, cache, G, N, P):
    p = _probe_problem(eng, cache, G, N)
    assert eng.list_params(N)[0] == 16
    lb = _labels(eng, orc, cache, (G, N), p, P)
    with _route(eng, "none", p, P):
        _edges_and_random(eng, p, lb, "lists")


def test_lists_sweep(eng, orc, cache):
    G, N, P = 300, 65, 129
    p = _probe_problem(eng, cache, G, N)
    lb = _labels(eng, orc, cache, (G, N), p, P)
    with _route(eng, "none", p, P):
        _sweep(eng, p, lb, "lists")


# ------------------------------------------------------------------ 3. the other list instantiations ------
@pytest.mark.parametrize("N,P,tw,segments", [(2600, 70, 8, 1), (5200, 70, 4, 1), (10_300, 70, 2, 1),
                                             (20_500, 40, 2, 2)])
def test_list_variants_edges_and_random(eng, orc, cache, N, P, tw, segments):
    """TW = 8 / 4 / 2 (12, 13, 14 counter planes) and k_permute_seglists; one-hots at isolate 0, the last
    isolate of the first segment, the first of the second, N - 1 (and the usual ones between)."""
    assert eng.list_params(N)[0] == tw and int(eng.lib.scoary_list_segments(N)) == segments
    G = 80
    p = _probe_problem(eng, cache, G, N, extra_hots=(pr.SEG_ROWS - 1, pr.SEG_ROWS))
    assert p.gm.lists.panels is None
    lb = _labels(eng, orc, cache, (G, N), p, P)
    with _route(eng, "none", p, P):
        _edges_and_random(eng, p, lb, "lists TW=%d segments=%d" % (tw, segments))


# ------------------------------------------------------------------ 4. dense k_permute ------
# tiled row size (quads) of the dense cases: every k_permute_reg instance (1, 2, 4, 6, 8, 12, 16, 20, 24 quads) and
# k_permute_chunked (> 24)
DENSE_ROW_QUADS = {65: 1, 200: 2, 400: 4, 700: 6, 1000: 8, 1300: 12, 1800: 16, 2300: 20, 2600: 24, 3300: 32}


@pytest.mark.parametrize("G,N,P", [(300, 65, 129), (513, 1000, 193), (60, 3300, 70)]
                         + [(60, N, 70) for N in (200, 400, 700, 1300, 1800, 2300, 2600)])
def test_dense_edges_and_random(eng, orc, cache, G, N, P):
    """scoary_permute with the gene-order form of the same intervals: every register row size (N <= 3072) and the
    chunked variant (N = 3300)."""
    import torch
    assert eng.quads(N) == DENSE_ROW_QUADS[N]           # which instance the shape reaches
    p = _probe_problem(eng, cache, G, N)
    lb = _labels(eng, orc, cache, (G, N), p, P, rows=True)
    for name, lo, hi1 in _families(p):
        lo, hi1 = pr.check_regions(lo, hi1, p.m)
        crit = torch.from_numpy(pr.gene_order_crit(lo, hi1, p.order, p.flipped, p.npos)).to(eng.device)
        r = torch.zeros((p.T, G), dtype=torch.int32, device=eng.device)
        eng.permute(p.gm, lb.rows, crit, r, P=P)
        got, want = _host(r), pr.r_ref(lb.u, p.order, lo, hi1)
        assert np.array_equal(got, want), _where(p, got, want, lo, hi1, "dense P=%d %s" % (P, name))


# ------------------------------------------------------------------ 5. k_lists_crit ------
@pytest.mark.parametrize("mode", ["all", "none"])
def test_gene_order_regions_through_k_lists_crit(eng, orc, cache, mode):
    G, N, P = 513, 1000, 193
    p = _probe_problem(eng, cache, G, N)
    lb = _labels(eng, orc, cache, (G, N), p, P)
    with _route(eng, mode, p, P):
        _edges_and_random(eng, p, lb, "k_lists_crit %s" % mode, crit=True)


# ------------------------------------------------------------------ 6. forced split ------
def _natural_regions(eng, p):
    """The slot-order intervals scoary_fisher_lists derives from the data."""
    _p, _odds, _crit, lcrit = eng.fisher(p.counts, lists=p.gm.lists)
    lc = lcrit.cpu().numpy().view(np.uint32).astype(np.int64)
    return lc[..., 0], lc[..., 1]


def _forced_split_case(eng, orc, cache, monkeypatch, G, N, P, k, with_empty, families):
    p = _probe_problem(eng, cache, G, N, T=3, with_empty=with_empty)
    assert p.gm.lists.panels is not None and 0 < k < G and k % 256 == 0
    a, b = p.order[k - 1], p.order[k]
    assert a != b and p.L[a] > 0 and p.L[b] > 0          # both sides of the hand-off carry a list
    lb = _labels(eng, orc, cache, (G, N, 3, with_empty), p, P)
    monkeypatch.setattr(eng, "mfma_split", lambda genes, T, P: k)
    fams = {"natural": _natural_regions(eng, p), "random": pr.random_regions(p.m, 3),
            "(0,0)": pr.edge_regions(p.m)["(0,0)"], "[0,m+1)": pr.edge_regions(p.m)["[0,m+1)"],
            "random 4": pr.random_regions(p.m, 4)}
    for name in families:
        lo, hi1 = fams[name]
        what = "split at %d, P=%d, %s" % (k, P, name)
        r, _got = _expect(eng, p, lb, lo, hi1, what)
        _expect(eng, p, lb, lo, hi1, what + ", second call accumulates", r=r, accumulate=True, factor=2)


@pytest.mark.parametrize("G,N,P,k,with_empty", [(1000, 1000, 193, 256, True), (1000, 1000, 193, 512, True),
                                                (1000, 1000, 193, 768, True), (513, 65, 129, 256, False),
                                                (513, 65, 129, 512, False), (512, 2048, 65, 256, True)])
def test_forced_split(eng, orc, cache, monkeypatch, G, N, P, k, with_empty):
    """Slots [0, k) on the matrix cores, [k, G) on the list walk, one k_lists_reduce over both: k below
    anything the routing picks by itself at these sizes.  (G = 513: without the absent and the core gene,
    whose empty lists would be the last slots.)"""
    _forced_split_case(eng, orc, cache, monkeypatch, G, N, P, k, with_empty, ("natural", "random", "(0,0)"))


# ------------------------------------------------------------------ 7. poisoned scratch ------
@pytest.mark.parametrize("k", [None, 256])
def test_poisoned_scratch_three_ranges(eng, orc, cache, monkeypatch, k):
    """P = 1100: 18 stages in three ranges per trait, three partial tiles; all routed, and split at 256."""
    G, N, P = 513, 1000, 1100
    fams = ("natural", "random", "random 4", "(0,0)", "[0,m+1)")
    if k is not None:
        _forced_split_case(eng, orc, cache, monkeypatch, G, N, P, k, True, fams)
        return
    p = _probe_problem(eng, cache, G, N, T=3)
    lb = _labels(eng, orc, cache, (G, N, 3, True), p, P)
    with _route(eng, "all", p, P):
        _edges_and_random(eng, p, lb, "poisoned scratch")
        lo, hi1 = _natural_regions(eng, p)
        _expect(eng, p, lb, lo, hi1, "poisoned scratch, natural")


def test_poisoned_scratch_tiles_beyond_the_ranges(eng, orc, cache):
    """P = 33 000: 65 partial tiles, but a trait has at most 64 ranges (here 58 of 9 stages): the tiles
    58 .. 64 are written by the zero fill of k_permute_mfma alone."""
    G, N, P = 33, 64, 33_000
    p = _probe_problem(eng, cache, G, N, T=3)
    lb = _labels(eng, orc, cache, (G, N, 3, True), p, P)
    with _route(eng, "all", p, P):
        for name in ("(0,0)", "[0,m+1)", "[0,1)"):
            lo, hi1 = pr.edge_regions(p.m)[name]
            _expect(eng, p, lb, lo, hi1, "P=%d %s" % (P, name))
        lo, hi1 = pr.random_regions(p.m, 5)
        _expect(eng, p, lb, lo, hi1, "P=%d random" % P)


# ------------------------------------------------------------------ 8. 16-bit range count ------
@pytest.mark.parametrize("P", [65_472, 65_473, 70_000])
def test_sixteen_bit_range_count(eng, cache, P):
    import torch
    if torch.cuda.get_device_properties(eng.device).multi_processor_count != 256:
        pytest.skip("the geometry keeps a 1023-stage range only where 256 blocks are one round over the CUs")
    G, N, T = 4096, 64, 16
    key = ("range16", G, N, T)
    p = cache.get(key)
    if p is None:
        rng = np.random.default_rng(31)
        traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
        traits[1, ::29] = 2
        traits[2, 5::17] = 2
        genes, _names = pr.probe_genes(G, N, traits, 31)
        p = _problem(eng, cache, key, genes, traits)
    assert -(-G // 256) * T == 256
    tiles = eng.perm_generate_tiles(p.mkv, p.margins, N, P, 0, 7)
    edges = pr.edge_regions(p.m)
    with _route(eng, "all", p, P):
        r = _lists_r(eng, p, tiles, P, *edges["(0,0)"])          # one call: the C ABI takes this P
        assert np.all(_host(r) == P)
        r = _lists_r(eng, p, tiles, P, *edges["[0,m+1)"])
        assert not _host(r).any()
        lo, hi1 = pr.random_regions(p.m, 6)
        got = _host(_lists_r(eng, p, tiles, P, lo, hi1))
    rows = eng.perm_generate(p.mkv, p.margins, N, P, 0, 7)
    crit = torch.from_numpy(pr.gene_order_crit(lo, hi1, p.order, p.flipped, p.npos)).to(eng.device)
    rd = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    eng.permute(p.gm, rows, crit, rd, P=P)
    want = _host(rd)
    assert np.array_equal(got, want), _where(p, got, want, lo, hi1, "P=%d random, against the dense kernel" % P)
    assert want.max() <= P and len(np.unique(want)) > 2
