"""The Fisher pass of the list path with one weight chain per margin class (scoary_fisher_lists_chained:
k_fisher_chains + k_fisher_tables) against the kernel it replaces (the handle switch, set_fisher_route("walk")) and
against the generic scoary_fisher: p, odds and both forms of the rejection region bit for bit, on the shapes where
the two-kernel pass takes a path of its own (forced with set_fisher_route("chains"): the default, "auto", keeps
launches this small on the one kernel) -- ties and double modes, supports that start above 0, tables that
walk past the end of a stored chain (floor, capacity), SciPy's small-N double, degenerate tables, the shortest
supports -- and one whole step, eager and replayed from a captured graph."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _three_ways(eng, genes, traits):
    """The tables of (genes, traits) through the chained pass, the one-kernel walk in slot order and the generic
    kernel: asserts that all outputs agree bit for bit, that the chained pass wrote its slabs and the walk did not
    touch them.  Returns (counts [T, G, 4], p [T, G], chain lengths [T, C, 2]) as numpy arrays."""
    import torch
    from scoary_amd.engine import pack_bits_rows
    genes = np.ascontiguousarray(genes, dtype=np.uint8)
    T, N = traits.shape
    gm = eng.pack_dense(genes)
    eng.build_lists(gm)
    trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
    mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
    counts, _margins = eng.counts(gm, trv, mkv)
    slabs = eng.fisher_chains(T, N)
    assert slabs is not None, "the chains of this shape must fit the budget"
    nlen = T * (N // 2) * 2

    slabs.fill_(-1)
    try:
        eng.set_fisher_route("chains")
        chained = eng.fisher(counts, lists=gm.lists)
        torch.cuda.synchronize()
        lens = slabs[:nlen].cpu().numpy().reshape(T, N // 2, 2)
        assert (lens >= 0).all() and (lens <= eng.lib.scoary_fisher_chains_capacity()).all()
        slabs.fill_(-1)
        eng.set_fisher_route("walk")
        walk = eng.fisher(counts, lists=gm.lists)
        torch.cuda.synchronize()
    finally:
        eng.set_fisher_route("auto")
    assert bool((slabs == -1).all()), "the walk route must not run the chain kernels"
    generic = eng.fisher(counts)

    def raw(t, dtype):
        return t.cpu().numpy().view(dtype)

    for name, other in (("walk", walk), ("generic", generic)):
        assert np.array_equal(raw(chained[0], np.uint64), raw(other[0], np.uint64)), "p vs " + name
        assert np.array_equal(raw(chained[1], np.int64), raw(other[1], np.int64)), "odds vs " + name
        assert np.array_equal(raw(chained[2], np.uint32), raw(other[2], np.uint32)), "crit vs " + name
    assert np.array_equal(raw(chained[3], np.uint32), raw(walk[3], np.uint32)), "lcrit vs walk"
    return counts.cpu().numpy(), chained[0].cpu().numpy(), lens


def _genes_with(trait, n, a_values, rng):
    """One gene per a: carried by n valid isolates of `trait`, a of them positives."""
    pos, neg = np.flatnonzero(trait == 1), np.flatnonzero(trait == 0)
    out = np.zeros((len(a_values), trait.size), dtype=np.uint8)
    for row, a in zip(out, a_values):
        row[rng.permutation(pos)[:a]] = 1
        row[rng.permutation(neg)[:n - a]] = 1
    return out


def test_random_case_missing_values_and_high_prevalence(eng):
    """3000 x 400 x 3: 1 % missing values in trait 0 (n varies inside a run of slots), prevalence 0.95 in trait 1
    (supports with lo > 0)."""
    rng = np.random.default_rng(20261019)
    G, N = 3000, 400
    genes = (rng.random((G, N)) < rng.uniform(0.01, 0.99, (G, 1))).astype(np.uint8)
    traits = np.stack([rng.random(N) < 0.4, rng.random(N) < 0.95, rng.random(N) < 0.25]).astype(np.uint8)
    traits[0, rng.permutation(N)[:N // 100]] = 2
    counts, p, lens = _three_ways(eng, genes, traits)
    n1, n = counts[1, :, 0] + counts[1, :, 1], counts[1, :, 0] + counts[1, :, 2]
    n2 = counts[1, :, 2] + counts[1, :, 3]
    assert (np.minimum(n, N - n) > n2).any(), "no support with lo > 0 among the tables of the 0.95 trait"
    assert len(np.unique(counts[0].sum(axis=1))) == 1 and counts[0, 0].sum() < N
    assert lens.max() > 1 and (p < 1).any()


@pytest.mark.parametrize("N", [200, 400])
def test_symmetric_margins_ties_and_double_modes(eng, N):
    """n1 == n2 with an even N: w(x) = w(n - x), so every table has an exact tie on the other side of the mode;
    genes carried by exactly half of the isolates (mirror rule, two equal modes) and by half +- 1, every a."""
    rng = np.random.default_rng(N)
    trait = np.zeros(N, dtype=np.uint8)
    trait[rng.permutation(N)[:N // 2]] = 1
    parts = [_genes_with(trait, n, range(max(0, n - N // 2), min(n, N // 2) + 1), rng)
             for n in (N // 2 - 1, N // 2, N // 2 + 1)]
    parts.append((rng.random((300, N)) < rng.uniform(0.02, 0.98, (300, 1))).astype(np.uint8))
    counts, p, _lens = _three_ways(eng, np.concatenate(parts), trait[None, :])
    assert (counts[0, :, 0] + counts[0, :, 1] == N // 2).all()
    assert (p == 1.0).any() and (p < 1e-30).any()


def _must_leave_chain(n1, n2, n, a, cap, floor):
    """True when a lane of the table (canonical margins n1, n2, n, observed a) certainly goes past the end of its
    stored chain: on one side, the first term below 2^-64 of the observed weight (the earliest the loop can end;
    or the end of the support) lies beyond the chain's last entry at the latest place that can be (the capacity, or
    the first weight below the floor).  Weights by lgamma, as log2 relative to the mode's, with one bit of slack
    on both thresholds for its error."""
    def lw(x):
        return -(math.lgamma(x + 1) + math.lgamma(n1 - x + 1) + math.lgamma(n - x + 1)
                 + math.lgamma(n2 - n + x + 1)) / math.log(2.0)
    lo, hi = max(0, n - n2), min(n, n1)
    mode = min(max(int((n + 1) * (n1 + 1) / (n1 + n2 + 2)), lo), hi)
    tiny = min(lw(a) - lw(mode), 0.0) - 64.0
    for xs in (range(mode, hi + 1), range(mode, lo - 1, -1)):
        w = np.array([lw(x) for x in xs]) - lw(mode)
        below_floor = np.flatnonzero(w < math.log2(floor) - 1.0)
        last = min(cap, len(w), below_floor[0] + 1 if len(below_floor) else len(w)) - 1   # index of the last entry
        stop = np.flatnonzero(w < tiny + 1.0)
        stop = stop[0] if len(stop) else len(w) - 1
        if stop > last:
            return True
    return False


def test_deep_tails_walk_past_the_end_of_a_chain(eng):
    """N = 2000: the trait row with 0, 1, 2, ... flipped isolates and the complements -- observed weights down to
    2^-1900 of the mode's, far below the floor the chains end at; the lanes go on by themselves from there."""
    rng = np.random.default_rng(7)
    N, K = 2000, 300
    trait = (rng.random(N) < 0.4).astype(np.uint8)
    genes = np.repeat(trait[None, :], K, axis=0)
    flip = rng.permutation(N)
    for k in range(K):
        genes[k, flip[:k]] ^= 1
    genes = np.concatenate([genes, 1 - genes])
    counts, p, lens = _three_ways(eng, genes, trait[None, :])
    cap, floor = int(eng.lib.scoary_fisher_chains_capacity()), float(eng.lib.scoary_fisher_chains_floor())
    assert cap >= 1 and 0.0 < floor < 1.0
    leave = 0
    for a, b, c, d in counts[0][::7]:
        n1, n2, n0 = int(a + b), int(c + d), int(a + c)
        mirrored = n0 > b + d or (n0 == b + d and a > b)
        leave += _must_leave_chain(n1, n2, int(b + d) if mirrored else n0, int(b) if mirrored else int(a), cap, floor)
    print("tables that must walk past the end of a stored chain: %d of %d looked at" % (leave, len(counts[0][::7])))
    assert leave > 0
    assert (p[0] < 1e-300).any()


@pytest.mark.parametrize("N", [131, 171])
def test_small_populations(eng, N):
    """N = 131: SciPy's own double overwrites p (the regions still come from the walk); N = 171: one trait with all
    isolates valid (the first size without it) and one with missing values (below it again)."""
    rng = np.random.default_rng(N)
    genes = (rng.random((800, N)) < rng.uniform(0.02, 0.98, (800, 1))).astype(np.uint8)
    traits = (rng.random((2, N)) < np.array([[0.35], [0.6]])).astype(np.uint8)
    traits[1, rng.random(N) < 0.05] = 2
    _three_ways(eng, genes, traits)


def test_degenerate_tables(eng):
    """Core genes (present in all / in no isolate), a trait whose positives are all missing and one without
    negatives: p = 1, odds = nan, empty regions, and classes of length 0."""
    rng = np.random.default_rng(3)
    G, N = 500, 300
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[:5], genes[5:10] = 0, 1
    traits = (rng.random((3, N)) < 0.4).astype(np.uint8)
    traits[1][traits[1] == 1] = 2
    traits[2][traits[2] == 0] = 2
    counts, p, lens = _three_ways(eng, genes, traits)
    assert (p[:, :10] == 1.0).all() and (p[1:] == 1.0).all()
    assert (lens[1:] == 0).all() and lens[0].max() > 1


def test_short_supports(eng):
    """n = 1, 2, 3 (and N - n: the mirrored orientation) and n = floor(Nvalid / 2), the last class of a trait with
    missing values; every a of each."""
    rng = np.random.default_rng(11)
    N = 401
    trait = (rng.random(N) < 0.3).astype(np.uint8)
    trait[rng.permutation(N)[:20]] = 2
    valid = np.flatnonzero(trait != 2)
    n1, nv = int((trait == 1).sum()), valid.size
    parts = []
    for n in (1, 2, 3, nv // 2):
        g = _genes_with(trait, n, range(max(0, n - (nv - n1)), min(n, n1) + 1), rng)
        comp = 1 - g
        comp[:, trait == 2] = rng.integers(0, 2, (len(g), N - nv))
        parts += [g, comp]
    counts, _p, lens = _three_ways(eng, np.concatenate(parts), trait[None, :])
    n = np.minimum(counts[0, :, 0] + counts[0, :, 2], counts[0, :, 1] + counts[0, :, 3])
    assert {1, 2, 3, nv // 2} == set(n.tolist())
    assert (lens[0, :nv // 2] > 0).all() and (lens[0, nv // 2:] == 0).all()


def test_support_longer_than_the_slab_capacity(eng):
    """N = 9000, one trait: supports of thousands of points, chains that end at the capacity long before the
    floor, so most lanes finish on their own walk."""
    rng = np.random.default_rng(9000)
    G, N = 400, 9000
    genes = (rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))).astype(np.uint8)
    trait = (rng.random(N) < 0.45).astype(np.uint8)
    _counts, p, lens = _three_ways(eng, genes, trait[None, :])
    assert lens.max() == eng.lib.scoary_fisher_chains_capacity()
    assert (p < 1).any()


def test_chains_bytes_and_budget(eng):
    """scoary_fisher_chains_bytes: 0 above the budget (cfg5's 10 000 isolates x 50 traits: evaluated, not run), a
    positive size at cfg3 and cfg4, and the engine follows it."""
    lib = eng.lib
    assert lib.scoary_fisher_chains_bytes(50, 10_000) == 0
    cfg3, cfg4 = lib.scoary_fisher_chains_bytes(10, 2_000), lib.scoary_fisher_chains_bytes(1, 5_000)
    cap = lib.scoary_fisher_chains_capacity()
    assert cfg3 >= 10 * 1000 * 2 * cap * 16 and cfg4 >= 2500 * 2 * cap * 16
    assert cfg3 <= 256 << 20 and cfg4 < cfg3
    assert lib.scoary_fisher_chains_bytes(0, 2_000) == 0 and lib.scoary_fisher_chains_bytes(1, 1) == 0
    assert eng.fisher_chains(50, 10_000) is None
    assert lib.scoary_set_fisher_route(eng.h, 3) != 0 and lib.scoary_set_fisher_route(eng.h, -1) != 0
    assert lib.scoary_set_fisher_route(eng.h, 2) == 0


def test_auto_route_takes_the_chains_from_four_wavefronts_per_simd(eng):
    """The default route: a launch of fewer than four table wavefronts per SIMD (128 tables per SIMD) leaves the
    slabs alone, one of that size fills them -- and its results, 140 000 tables of one trait in several hundred
    blocks, are the walk's bit for bit.  Tables made directly: every a of the support of random counts n."""
    import torch
    from scoary_amd.engine import GeneLists
    rng = np.random.default_rng(140)
    N, n1 = 400, 150
    simds = 4 * torch.cuda.get_device_properties(eng.device).multi_processor_count
    outs = {}
    for G in (64 * simds, 128 * simds + 7):
        n = rng.integers(0, N + 1, G)
        a = rng.integers(np.maximum(0, n - (N - n1)), np.minimum(n, n1) + 1)
        tabs = np.stack([a, n1 - a, n - a, N - n1 - n + a], axis=1).astype(np.int32)
        assert (tabs >= 0).all()
        counts = torch.from_numpy(tabs[None]).to(eng.device)
        order = torch.from_numpy(np.argsort(-np.minimum(n, N - n), kind="stable").astype(np.int32)).to(eng.device)
        flipped = torch.from_numpy((2 * n > N).astype(np.uint8)).to(eng.device)
        lists = GeneLists(None, None, None, order, flipped, 0, N)
        slabs = eng.fisher_chains(1, N)
        slabs.fill_(-1)
        outs[G] = eng.fisher(counts, lists=lists)
        torch.cuda.synchronize()
        assert bool((slabs[:N] >= 0).all()) == (G >= 128 * simds), G
    G = 128 * simds + 7
    eng.set_fisher_route("walk")
    try:
        walk = eng.fisher(counts, lists=lists)
    finally:
        eng.set_fisher_route("auto")
    for got, want in zip(outs[G], walk):
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


def test_whole_step_eager_and_captured(eng):
    """One small step (900 x 400 x 2, P = 700) with the chained pass: r is the oracle's, and the step replayed
    from a captured graph returns the eager step's p, odds, regions and r bit for bit."""
    from scoary_amd.engine import pack_bits_rows
    rng = np.random.default_rng(900)
    G, N, T, P, seed = 900, 400, 2, 700, 41
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    traits[1, ::37] = 2
    tb, mb = pack_bits_rows((traits == 1).astype(np.uint8)), pack_bits_rows((traits != 2).astype(np.uint8))
    gm = eng.pack_dense(genes)
    eng.build_lists(gm)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    slabs = eng.fisher_chains(T, N)
    slabs.fill_(-1)
    eng.set_fisher_route("chains")
    try:
        _whole_step(eng, gm, trv, mkv, slabs, genes, tb, mb, T, N, P, seed)
    finally:
        eng.set_fisher_route("auto")


def _whole_step(eng, gm, trv, mkv, slabs, genes, tb, mb, T, N, P, seed):
    import torch
    from oracle import oracle as orc
    eager = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True)
    torch.cuda.synchronize()
    assert bool((slabs[:T * (N // 2) * 2] >= 0).all()), "the step did not run the chained pass"
    want = {k: eager[k].cpu().numpy().copy() for k in ("p", "odds", "crit", "r")}
    r = orc.permute_r(orc.pack_rows(genes), tb, mb, N, P, seed).T
    assert np.array_equal(want["r"].view(np.uint32), r)

    ws = eng.workspace(gm, T, P, use_lists=True)
    plan = eng.trait_plan(trv, mkv, N)
    graph, res = eng.capture(gm, trv, mkv, P, seed, ws, use_lists=True, plan=plan)
    for k in want:
        res[k].zero_()
    slabs.fill_(-1)
    graph.launch()
    torch.cuda.synchronize()
    assert bool((slabs[:T * (N // 2) * 2] >= 0).all())
    for k in want:
        assert res[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    graph.close()
