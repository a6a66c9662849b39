"""GPU parity: the HIP path (through the C-ABI) against the CPU oracle and the
reference's golden vectors.  Bit-exact for counts / packing / permutation
labels / exceedance counts; |dp| < 1e-12 for Fisher p (north_star tolerance).
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_text, read_dense

pytestmark = pytest.mark.gpu

P_TOL = 1e-12   # BASELINE.json north_star: Fisher / empirical p within 1e-12


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _bits(eng, traits):
    from scoary_amd.engine import pack_bits_rows
    tb = pack_bits_rows((traits == 1).astype(np.uint8))
    mb = pack_bits_rows((traits != 2).astype(np.uint8))
    return tb, mb


def _tiled_to_rows(tiled, G, N):
    """Undo the tiled layout on the host: [Qp, Gp, 4] int32 -> (G, W64) uint64."""
    t = tiled.cpu().numpy().view(np.uint32)            # Qp, Gp, 4
    Qp, Gp, _ = t.shape
    rows32 = t.transpose(1, 0, 2).reshape(Gp, Qp * 4)
    W = (N + 63) // 64
    assert not rows32[G:].any(), "padding genes must be zero"
    assert not rows32[:, 2 * W:].any(), "padding words must be zero"
    return np.ascontiguousarray(rows32[:G, :2 * W]).view(np.uint64)


def _random_case(rng, G, N, T, missing=True):
    genes = (rng.random((G, N)) < rng.uniform(0.01, 0.99, (G, 1))).astype(np.uint8)
    if G > 4:
        genes[1] = 0
        genes[2] = 1
    traits = (rng.random((T, N)) < rng.uniform(0.15, 0.85, (T, 1))).astype(np.uint8)
    if missing:
        for t in range(0, T, 2):
            traits[t, rng.random(N) < 0.05] = 2
    return genes, traits


# ------------------------------------------------------------------ a1 ------
@pytest.mark.parametrize("G,N", [(1, 1), (5, 31), (64, 32), (257, 33), (300, 64), (1000, 65),
                                 (77, 127), (513, 128), (40, 500), (33, 2000), (9, 6200)])
def test_pack_dense_and_tile_rows_bit_exact(eng, orc, G, N):
    rng = np.random.default_rng(G * 7919 + N)
    genes = (rng.random((G, N)) < 0.5).astype(np.uint8)
    want = orc.pack_rows(genes)
    gm = eng.pack_dense(genes * rng.integers(1, 255, size=genes.shape, dtype=np.uint8))
    assert np.array_equal(_tiled_to_rows(gm.tiled, G, N), want)
    from scoary_amd.engine import pack_bits_rows
    assert np.array_equal(pack_bits_rows(genes), want)
    gm2 = eng.tile_rows(want, N)
    assert np.array_equal(gm2.tiled.cpu().numpy(), gm.tiled.cpu().numpy())


# ------------------------------------------------------------------ a3 ------
@pytest.mark.parametrize("G,N,T", [(1, 1, 1), (3, 5, 2), (100, 64, 1), (257, 100, 5), (1000, 129, 9),
                                   (4097, 500, 4), (600, 2000, 10), (130, 5000, 3),
                                   (70, 10000, 2)])
def test_counts_bit_exact(eng, orc, G, N, T):
    rng = np.random.default_rng(G + 31 * N + 977 * T)
    genes, traits = _random_case(rng, G, N, T)
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    counts, margins = eng.counts(gm, eng.vecrows(tb, N), eng.vecrows(mb, N))
    got = counts.cpu().numpy()
    # the isolate-by-isolate restatement of Perform_statistics
    for t in range(T):
        assert np.array_equal(got[t], orc.counts_dense(genes, traits[t])), "trait %d" % t
    m = margins.cpu().numpy()
    assert np.array_equal(m[:, 0], (traits == 1).sum(1))
    assert np.array_equal(m[:, 1], (traits != 2).sum(1))


@pytest.mark.parametrize("G,N,T,pattern", [(300, 333, 50, "shared"), (130, 700, 70, "mixed"), (65, 129, 33, "distinct"),
                                           (1000, 64, 17, "mixed"), (64, 10000, 50, "shared"), (500, 2000, 4, "mixed")])
def test_counts_one_pass_many_traits_and_mask_classes(eng, orc, G, N, T, pattern):
    """K1, round 4: up to 32 traits per pass over the gene matrix (T = 50:
    two balanced passes of 25, T = 70: three), the quads of a row split over four wavefronts and
    reduced in LDS, and popc(gene & valid) counted once per class of identical validity rows
    (scoary_trait_plan) -- against the isolate-by-isolate restatement of Perform_statistics
    (scoary/methods.py:940-965) for every (gene, trait); the plan's classes against numpy; and
    the one-call scoary_counts (no classes) bit-identical to the planned call."""
    import ctypes
    import torch
    rng = np.random.default_rng(G + N + T)
    genes, traits = _random_case(rng, G, N, T, missing=False)
    if pattern == "shared":                                   # like cfg3 / cfg5: two traits with missing values
        for t in (T - 2, T - 1):
            traits[t, rng.random(N) < 0.01] = 2
    elif pattern == "distinct":                               # every trait its own mask
        for t in range(T):
            traits[t, rng.random(N) < 0.05] = 2
    else:                                                     # a few masks, shared in an irregular order
        holes = [rng.random(N) < 0.04 for _ in range(3)]
        for t in range(T):
            k = int(rng.integers(0, 4))
            if k < 3:
                traits[t, holes[k]] = 2
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    plan = eng.trait_plan(trv, mkv, N)
    valid = traits != 2
    tpp = int(eng.lib.scoary_counts_traits_per_pass(T))          # classes are shared within a pass
    want_cls = np.array([min(u for u in range(t // tpp * tpp, t + 1) if np.array_equal(valid[u], valid[t]))
                         for t in range(T)])
    assert np.array_equal(plan.mask_class.cpu().numpy(), want_cls)
    m = plan.margins.cpu().numpy()
    assert np.array_equal(m[:, 0], (traits == 1).sum(1)) and np.array_equal(m[:, 1], valid.sum(1))
    counts, margins = eng.counts(gm, trv, mkv, plan=plan)
    got = counts.cpu().numpy()
    want = np.stack([orc.counts_dense(genes, traits[t]) for t in range(T)])
    assert np.array_equal(got, want)
    # the one-call form of the C-ABI: plan (without classes) + tables
    c2 = torch.full((T, G, 4), -7, dtype=torch.int32, device=eng.device)
    m2 = torch.zeros((T, 2), dtype=torch.int32, device=eng.device)
    vp = ctypes.c_void_p
    rc = eng.lib.scoary_counts(eng.h, vp(gm.tiled.data_ptr()), vp(trv.data_ptr()), vp(mkv.data_ptr()), G, T, N,
                               vp(c2.data_ptr()), vp(m2.data_ptr()), eng._stream())
    assert rc == 0 and torch.equal(c2, counts) and torch.equal(m2, plan.margins)
    with pytest.raises(ValueError):                           # a plan belongs to the tensors it was built from
        eng.counts(gm, trv.clone(), mkv, plan=plan)


def test_counts_all_missing_and_constant_traits(eng, orc):
    rng = np.random.default_rng(4)
    genes, _ = _random_case(rng, 200, 150, 1)
    traits = np.zeros((4, 150), dtype=np.uint8)
    traits[1] = 1
    traits[2] = 2                      # every isolate missing
    traits[3, :75] = 1
    tb, mb = _bits(eng, traits)
    counts, _ = eng.counts(eng.pack_dense(genes), eng.vecrows(tb, 150), eng.vecrows(mb, 150))
    got = counts.cpu().numpy()
    for t in range(4):
        assert np.array_equal(got[t], orc.counts_dense(genes, traits[t]))
    assert not got[2].any()


def test_counts_exampledata_golden(eng):
    """All 9001 x 2 (gene, trait) tallies of the reference's exampledata, incl.
    Bogus_trait's missing values, against Setup_results captured from the
    reference."""
    ids, strains, genes, names, traits = read_dense(
        golden_text("exampledata/Gene_presence_absence.csv.gz"),
        golden_text("exampledata/Tetracycline_resistance.csv.gz"))
    z = np.load(os.path.join(GOLDEN, "setup_results_exampledata.npz"))
    tb, mb = _bits(eng, traits)
    N = len(strains)
    counts, _ = eng.counts(eng.pack_dense(genes), eng.vecrows(tb, N), eng.vecrows(mb, N))
    got = counts.cpu().numpy()
    for t in range(2):
        ggenes = json.loads(str(z["t%d_genes" % t]))
        idx = np.array([ids.index(g) for g in ggenes])
        assert np.array_equal(got[t][idx], z["t%d_counts" % t])
        # everything not in the golden set is a gene the reference skipped
        skipped = np.setdiff1d(np.arange(len(ids)), idx)
        c = got[t][skipped]
        assert np.all((c[:, 0] + c[:, 2] == 0) | (c[:, 1] + c[:, 3] == 0))


# ------------------------------------------------------------------ a5 ------
def test_fisher_golden_grid(eng):
    import torch
    z = np.load(os.path.join(GOLDEN, "fisher_grid.npz"))
    tabs = torch.from_numpy(z["tables"].astype(np.int32)).cuda()
    p, odds, crit = eng.fisher(tabs)
    p, odds = p.cpu().numpy(), odds.cpu().numpy()
    gp, go = z["p"], z["odds"]
    assert np.max(np.abs(p - gp)) < P_TOL
    big = gp > 1e-290
    assert np.max(np.abs(p[big] - gp[big]) / gp[big]) < 1e-10
    assert np.array_equal(np.isnan(odds), np.isnan(go))
    assert np.array_equal(np.isinf(odds), np.isinf(go))
    fin = np.isfinite(go)
    assert np.array_equal(odds[fin], go[fin])
    assert np.all(p[np.isnan(go)] == 1.0)


def test_fisher_vs_oracle_and_rejection_region(eng, orc):
    """p within 1e-12 of the oracle; the (base, span) rejection region equals
    the set {x : w(x) <= w(a_obs)(1 + 1e-14)} computed from the oracle's p-values."""
    import torch
    rng = np.random.default_rng(12)
    tabs = []
    for N in (12, 90, 700, 4000):
        for _ in range(150):
            n1 = int(rng.integers(1, N)); n = int(rng.integers(1, N))
            lo, hi = max(0, n - (N - n1)), min(n, n1)
            a = int(rng.integers(lo, hi + 1))
            tabs.append((a, n1 - a, n - a, N - n1 - n + a))
    tabs = np.array(tabs, dtype=np.int32)
    p, odds, crit = eng.fisher(torch.from_numpy(tabs).cuda())
    p = p.cpu().numpy()
    crit = crit.cpu().numpy().view(np.uint32)
    o_or, o_p = orc.fisher_many(tabs)
    assert np.max(np.abs(p - o_p)) < P_TOL
    for k in range(0, len(tabs), 7):
        a, b, c, d = (int(x) for x in tabs[k])
        n1, n2, n = a + b, c + d, a + c
        lo, hi = max(0, n - n2), min(n, n1)
        base, span = int(crit[k, 0]), int(crit[k, 1])
        if o_p[k] < 1e-280:
            continue        # p underflows: the p-based restatement of the region is void
        for x in range(lo, hi + 1):
            _, px = orc.fisher(x, n1 - x, n - x, n2 - n + x)
            in_region = ((x - base) % (1 << 32)) >= span
            assert in_region == (px <= o_p[k] * (1 + 1e-9)), (tabs[k], x, base, span)


def test_fisher_small_populations_equal_scipy_bit_for_bit(eng, orc):
    """N <= 170: k_fisher returns SciPy's own double (spec S3; the golden grid and the reference's exampledata
    p-values directly, every table up to N = 14 and random ones up to 170 through the pinned oracle); the
    region is still the exact rule's."""
    import torch
    z = np.load(os.path.join(GOLDEN, "fisher_grid.npz"))
    tabs, gp = z["tables"].astype(np.int32), z["p"]
    small = tabs.sum(1) <= 170
    p, _, _ = eng.fisher(torch.from_numpy(tabs[small]).cuda())
    assert np.array_equal(p.cpu().numpy().view(np.uint64), gp[small].view(np.uint64))
    for f, nt in (("setup_results_exampledata.npz", 2), ("setup_results_collapse.npz", 1),
                  ("setup_results_restrict.npz", 2), ("setup_results_vcf.npz", 1)):
        g = np.load(os.path.join(GOLDEN, f))
        for ti in range(nt):
            c = g["t%d_counts" % ti].astype(np.int32)
            p, _, _ = eng.fisher(torch.from_numpy(c).cuda(), want_crit=False)
            assert np.array_equal(p.cpu().numpy().view(np.uint64), g["t%d_p_v" % ti].view(np.uint64)), (f, ti)
    rng = np.random.default_rng(171)
    tabs = [(a, n1 - a, n - a, N - n1 - n + a) for N in range(2, 15) for n1 in range(1, N) for n in range(1, N)
            for a in range(max(0, n - (N - n1)), min(n, n1) + 1)]
    for N in (15, 33, 64, 101, 150, 169, 170):
        for _ in range(400):
            n1 = int(rng.integers(1, N)); n = int(rng.integers(1, N))
            a = int(rng.integers(max(0, n - (N - n1)), min(n, n1) + 1))
            tabs.append((a, n1 - a, n - a, N - n1 - n + a))
    tabs = np.array(tabs, dtype=np.int32)
    p, _, crit = eng.fisher(torch.from_numpy(tabs).cuda())
    _, o_p = orc.fisher_many(tabs)
    assert np.array_equal(p.cpu().numpy().view(np.uint64), o_p.view(np.uint64))
    # N = 171 is the first population on the other side: the walk's p, within the tolerance
    t171 = np.array([(30, 40, 50, 51), (1, 69, 99, 2), (35, 35, 50, 51)], dtype=np.int32)
    p, _, _ = eng.fisher(torch.from_numpy(t171).cuda())
    _, o_p = orc.fisher_many(t171)
    assert np.max(np.abs(p.cpu().numpy() - o_p) / o_p) < 1e-11


def test_fisher_scipy_digits_at_any_size(eng, orc):
    """scoary_fisher_scipy (k_fisher_scipy, what the command line prints above 170 isolates): SciPy's own double,
    bit for bit -- against the golden grid (every table above N = 170: SciPy 1.15.3), against the oracle's
    restatement of Boost's prime-factorised pmf on 12 000 random tables up to 104 723 isolates, and against the
    SciPy installed on this box; tables below 171 isolates, with an empty margin or above the maximum are left as
    scoary_fisher wrote them, the last kind counted."""
    import torch
    z = np.load(os.path.join(GOLDEN, "fisher_grid.npz"))
    tabs, gp = z["tables"].astype(np.int32), z["p"]
    dt = torch.from_numpy(tabs).to(eng.device)
    p = eng.fisher(dt)[0]
    assert eng.fisher_scipy(dt, p) == 0
    assert np.array_equal(p.cpu().numpy().view(np.uint64), gp.view(np.uint64))       # the whole grid, N <= 170 included
    rng = np.random.default_rng(2026)
    rand = []
    for k in range(12000):
        N = int(rng.choice([171, 200, 997, 2000, 5000, 10007, 40000, 104723])) if k % 3 == 0 else int(rng.integers(2, 12000))
        npos, g = int(rng.integers(1, N)), int(rng.integers(1, N))
        lo, hi = max(0, g + npos - N), min(g, npos)
        mu = g * npos / N
        sd = max(1.0, (mu * (1 - npos / N)) ** 0.5)
        a = int(min(max(round(mu + rng.normal() * sd * rng.choice([0.3, 1, 3, 10])), lo), hi))
        rand.append((a, npos - a, g - a, N - npos - g + a))
    rand += [(60000, 20000, 20000, 20000), (70000, 20000, 20000, 20000), (0, 0, 100, 200), (5, 0, 300, 0)]
    rand = np.array(rand, dtype=np.int32)
    dt = torch.from_numpy(rand).to(eng.device)
    walk = eng.fisher(dt)[0]
    p = walk.clone()
    assert eng.fisher_scipy(dt, p) == 2                                               # the two tables above the maximum
    got, walk = p.cpu().numpy(), walk.cpu().numpy()
    n = rand.sum(1)
    margins = np.minimum(np.minimum(rand[:, 0] + rand[:, 1], rand[:, 2] + rand[:, 3]),
                         np.minimum(rand[:, 0] + rand[:, 2], rand[:, 1] + rand[:, 3]))
    inside = (n >= 171) & (n <= eng.fisher_scipy_max_isolates()) & (margins > 0)
    assert inside.sum() > 11000
    want = orc.fisher_scipy_many(rand)
    assert np.array_equal(got[inside].view(np.uint64), want[inside].view(np.uint64))
    assert np.array_equal(got[~inside].view(np.uint64), walk[~inside].view(np.uint64))
    assert np.max(np.abs(walk[inside] - want[inside])) < 1e-12                         # and the walk is within the path's 1e-12
    ss = pytest.importorskip("scipy.stats")
    for k in np.nonzero(inside)[0][:600]:
        a, b, c, d = rand[k].tolist()
        assert got[k] == float(ss.fisher_exact([[a, b], [c, d]])[1]), rand[k]


def test_fisher_of_a_gene_and_of_its_complement_are_the_same_double(eng, orc):
    """[[a, b], [c, d]] and [[b, a], [d, c]] (a gene / the complementary gene under one trait): the same
    p bit for bit -- as SciPy returns for tables beyond its factorial table (N > 170), which is what keeps
    such rows in file order in the reference's CSV -- the same odds ratio reciprocal-wise, and regions
    that are each other's image under x -> n1 - x; both orientations still equal the oracle's regions."""
    import torch
    rng = np.random.default_rng(77)
    tabs = []
    for N in (171, 300, 500, 2000, 9000):               # (up to 170 the p is SciPy's, mirror noise included)
        for _ in range(120):
            n1 = int(rng.integers(1, N)); n = int(rng.integers(1, N))
            lo, hi = max(0, n - (N - n1)), min(n, n1)
            a = int(rng.integers(lo, hi + 1))
            tabs.append((a, n1 - a, n - a, N - n1 - n + a))
        tabs.append((N // 4, N // 4, N // 4, N - 3 * (N // 4)))          # gene carried by exactly half
        tabs.append((N // 4 - 1, N // 4 + 1, N // 4 + 1, N - 3 * (N // 4) - 1))
    tabs = np.array(tabs, dtype=np.int32)
    comp = tabs[:, [1, 0, 3, 2]].copy()
    p, odds, crit = eng.fisher(torch.from_numpy(tabs).cuda())
    pc, oddsc, critc = eng.fisher(torch.from_numpy(comp).cuda())
    p, pc = p.cpu().numpy(), pc.cpu().numpy()
    assert np.array_equal(p.view(np.uint64), pc.view(np.uint64))
    crit, critc = crit.cpu().numpy().view(np.uint32).astype(np.int64), critc.cpu().numpy().view(np.uint32).astype(np.int64)
    n1 = tabs[:, 0].astype(np.int64) + tabs[:, 1]
    some = crit[:, 1] > 0
    assert np.array_equal(some, critc[:, 1] > 0) and np.array_equal(crit[some, 1], critc[some, 1])
    # accept [base, base + span) in a  <=>  accept [n1 - base - span + 1, n1 - base + 1) in b = n1 - a
    assert np.array_equal(critc[some, 0], n1[some] - crit[some, 0] - crit[some, 1] + 1)
    _, o_p = orc.fisher_many(tabs)
    big = o_p > 1e-280                                   # below: p underflows on both sides
    assert np.max(np.abs(p - o_p)) < P_TOL and np.max(np.abs(p[big] - o_p[big]) / o_p[big]) < 1e-11


def test_fisher_exampledata_golden_p(eng):
    import torch
    z = np.load(os.path.join(GOLDEN, "setup_results_exampledata.npz"))
    for t in range(2):
        c = z["t%d_counts" % t]
        p, odds, _ = eng.fisher(torch.from_numpy(c).cuda(), want_crit=False)
        p, odds = p.cpu().numpy(), odds.cpu().numpy()
        gp, go = z["t%d_p_v" % t], z["t%d_OR" % t]
        assert np.max(np.abs(p - gp)) < P_TOL
        assert np.max(np.abs(p - gp) / gp) < 1e-11
        assert np.array_equal(odds[np.isfinite(go)], go[np.isfinite(go)])
    # the row the reference's own test pins, at the reference's own tolerance
    p, odds, _ = eng.fisher(torch.tensor([[29, 3, 8, 60]], dtype=torch.int32).cuda())
    assert abs(float(p[0]) - 1.08621066108e-14) < 1e-15
    assert abs(float(odds[0]) - 72.5) < 0.1


# ------------------------------------------------------------------ a8 ------
@pytest.mark.parametrize("N,T,P,base", [(1, 1, 3, 0), (63, 2, 70, 0), (64, 1, 65, 5), (500, 3, 130, 1000),
                                        (2000, 2, 64, 9990), (5000, 1, 10, 0)])
def test_perm_labels_bit_exact(eng, orc, N, T, P, base):
    rng = np.random.default_rng(N + T)
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    traits[0, rng.random(N) < 0.1] = 2
    tb, mb = _bits(eng, traits)
    masks = eng.vecrows(mb, N)
    trv = eng.vecrows(tb, N)
    gm = eng.pack_dense(np.ones((1, N), dtype=np.uint8))
    _, margins = eng.counts(gm, trv, masks)
    seed = 0xDEADBEEF12345678
    perms = eng.perm_generate(masks, margins, N, P, base, seed).cpu().numpy().view(np.uint32)
    W = (N + 63) // 64
    for t in range(T):
        npos = int((traits[t] == 1).sum())
        for j in (0, 1, P // 2, P - 1):
            want = orc.perm_labels(seed, t, base + j, mb[t], npos, N)
            got = np.ascontiguousarray(perms[t, j, :2 * W]).view(np.uint64)
            assert np.array_equal(got, want), (t, j)
            assert not perms[t, j, 2 * W:].any()


# ------------------------------------------------------------------ a7 ------
@pytest.mark.parametrize("G,N,T,P", [
    (1, 1, 1, 10), (70, 40, 2, 64), (300, 100, 2, 100), (513, 130, 3, 77),
    (1000, 500, 1, 300),      # cfg2 shape, reduced
    (400, 700, 2, 65), (300, 1000, 2, 64), (260, 1500, 1, 70),
    (500, 2000, 3, 150),      # cfg3 shape, reduced
    (200, 2500, 1, 64), (150, 3000, 1, 64), (130, 4000, 2, 64), (100, 5000, 1, 70),
    (90, 6100, 1, 64),
    (70, 7000, 1, 66),        # chunked kernel (row too long for registers)
    (64, 10000, 2, 64),       # cfg5 row length
])
def test_permute_r_bit_exact(eng, orc, G, N, T, P):
    rng = np.random.default_rng(G + N + P)
    genes, traits = _random_case(rng, G, N, T)
    tb, mb = _bits(eng, traits)
    seed = 424242 + N
    res = eng.associate(eng.pack_dense(genes), eng.vecrows(tb, N), eng.vecrows(mb, N),
                        permutations=P, seed=seed)
    got = res["r"].cpu().numpy().view(np.uint32)
    want = orc.permute_r(orc.pack_rows(genes), tb, mb, N, P, seed).T
    assert np.array_equal(got, want)
    assert got.max() <= P


def test_permute_batched_equals_single_shot(eng, orc):
    """Permutation indices are global: generating in batches (perm_base) gives
    the same exceedance counts as one shot -- and the same as the oracle."""
    import torch
    rng = np.random.default_rng(8)
    G, N, T, P = 300, 200, 2, 200
    genes, traits = _random_case(rng, G, N, T)
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    trv, mk = eng.vecrows(tb, N), eng.vecrows(mb, N)
    one = eng.associate(gm, trv, mk, permutations=P, seed=5)["r"].cpu().numpy()
    buf = torch.empty((T, 64, eng.row_words(N)), dtype=torch.int32, device="cuda")
    many = eng.associate(gm, trv, mk, permutations=P, seed=5, perm_buffer=buf)["r"].cpu().numpy()
    assert np.array_equal(one, many)
    want = orc.permute_r(orc.pack_rows(genes), tb, mb, N, P, 5).T
    assert np.array_equal(one.view(np.uint32), want)


def test_headline_config_properties(eng, orc):
    """BASELINE configs[2] at FULL size (50k x 2000 x 10, P reduced to keep the
    oracle leg short is NOT done here -- this test uses size-independent
    properties instead):
      * sum over the 2x2 cells == valid isolates of the trait, for every gene;
      * row/col margins are permutation invariant, so r <= P and
        r == P exactly for genes the reference skips;
      * a gene's complement has the same p and the same r (the test is
        symmetric under relabelling present/absent);
      * duplicated genes get identical results (idempotence across lanes);
      * the list-driven kernel (the bench default) and the dense kernel give the
        same r for all 500 000 (gene, trait) pairs;
      * a subsample of genes is checked bit-exactly against the oracle."""
    from scoary_amd import synth
    genes, traits, P_full, seed = synth.make_config("cfg3")
    G, N = genes.shape
    T = traits.shape[0]
    P = 256
    genes[101] = genes[100]                 # duplicate
    genes[103] = 1 - genes[102]             # complement
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    res = eng.associate(gm, eng.vecrows(tb, N), eng.vecrows(mb, N), permutations=P, seed=seed,
                        use_lists=False)
    eng.build_lists(gm)
    res_l = eng.associate(gm, eng.vecrows(tb, N), eng.vecrows(mb, N), permutations=P, seed=seed,
                          use_lists=True)
    assert np.array_equal(res_l["r"].cpu().numpy(), res["r"].cpu().numpy())
    counts = res["counts"].cpu().numpy()
    r = res["r"].cpu().numpy().view(np.uint32)
    p = res["p"].cpu().numpy()
    nval = (traits != 2).sum(1)
    assert np.array_equal(counts.sum(2), np.broadcast_to(nval[:, None], (T, G)))
    assert r.max() <= P
    skipped = (counts[:, :, 0] + counts[:, :, 2] == 0) | (counts[:, :, 1] + counts[:, :, 3] == 0)
    assert skipped.sum() > 0 and np.all(r[skipped] == P)
    assert np.array_equal(r[:, 100], r[:, 101]) and np.array_equal(p[:, 100], p[:, 101])
    assert np.array_equal(r[:, 102], r[:, 103])
    assert np.max(np.abs(p[:, 102] - p[:, 103])) < P_TOL
    # oracle on a stratified subsample (every 97th gene, all traits)
    sub = np.arange(0, G, 97)
    gb = orc.pack_rows(genes[sub])
    want_c = orc.counts_packed(gb, tb, mb).transpose(1, 0, 2)
    assert np.array_equal(counts[:, sub], want_c)
    _, want_p = orc.fisher_many(want_c.reshape(-1, 4))
    assert np.max(np.abs(p[:, sub].ravel() - want_p)) < P_TOL
    want_r = orc.permute_r(gb, tb, mb, N, P, seed).T
    assert np.array_equal(r[:, sub], want_r)


# ------------------------------------------------------ a7, list-driven -----
@pytest.mark.parametrize("G,N,T,P", [
    (1, 1, 1, 10), (7, 40, 2, 33), (300, 100, 2, 512), (513, 130, 3, 600), (1000, 500, 1, 1100),
    (400, 700, 2, 65), (260, 1500, 1, 700), (500, 2000, 3, 1030), (90, 2400, 2, 520),
    (64, 2559, 1, 513), (70, 2560, 1, 300), (130, 3000, 2, 260), (200, 4000, 1, 530),
    (90, 5000, 2, 257), (40, 5119, 1, 100),          # 8-dword tile rows, tiles of 256
    (50, 5120, 1, 129), (120, 7000, 2, 200), (70, 10000, 1, 130), (33, 10239, 1, 64),   # 4-dword
    (40, 10240, 1, 65), (130, 12001, 2, 130), (70, 16000, 1, 200), (65, 20479, 1, 64),   # 2-dword, two words per lane
    (40, 20480, 1, 33), (100, 30001, 2, 70), (65, 40959, 1, 32),     # 2-dword tiles in 2 / 2 / 3 isolate segments
])
def test_permute_lists_equals_dense_and_oracle(eng, orc, G, N, T, P):
    """The list-driven kernel (minority lists + bit-sliced counters) gives
    bit-identical exceedance counts to the dense kernel and to the oracle,
    including genes present everywhere / nowhere, dense genes (zeros-list),
    missing isolates and ragged last tiles."""
    rng = np.random.default_rng(G * 3 + N + P)
    genes, traits = _random_case(rng, G, N, T)
    if G > 20:
        genes[5] = (rng.random(N) < 0.97).astype(np.uint8)     # zeros-list, short
        genes[6] = (rng.random(N) < 0.02).astype(np.uint8)     # ones-list, short
        genes[7] = genes[8]                                    # duplicates
    tb, mb = _bits(eng, traits)
    from scoary_amd.engine import pack_bits_rows
    gm = eng.pack_dense(genes)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    seed = 99 + N
    dense = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=False)["r"].cpu().numpy()
    eng.build_lists(gm)
    assert eng.lists_supported(N)
    lists = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=True)["r"].cpu().numpy()
    assert np.array_equal(lists, dense)
    want = orc.permute_r(orc.pack_rows(genes), tb, mb, N, P, seed).T
    assert np.array_equal(lists.view(np.uint32), want)


@pytest.mark.parametrize("N,T,P", [(333, 2, 700), (2700, 2, 700), (6000, 2, 700), (64, 1, 64),
                                   (333, 4, 17000), (100, 3, 180000), (12001, 2, 130),
                                   (20479, 1, 70)])
def test_perm_tiles_are_the_transposed_row_labels(eng, N, T, P):
    """scoary_perm_generate_tiles writes the same spec-S4 labels as scoary_perm_generate,
    isolate-major in tiles of 512 / 256 / 128 / 64 permutations, zero row + zero ragged
    tail (the segmented tiles of N > 20479: test_segmented_list_path_vs_dense_and_oracle).
    The cases cover one, two and four dword columns per block (few / many (trait, tile)
    pairs) and 256 ... 1024 threads per block.  Tiles start at a multiple of 32 permutations;
    the row form takes any base (test_perm_labels_bit_exact)."""
    rng = np.random.default_rng(2)
    base = 64
    traits = (rng.random((T, N)) < 0.4).astype(np.uint8)
    traits[T - 1, rng.random(N) < 0.1] = 2
    tb, mb = _bits(eng, traits)
    masks, trv = eng.vecrows(mb, N), eng.vecrows(tb, N)
    _, margins = eng.counts(eng.pack_dense(np.ones((1, N), dtype=np.uint8)), trv, masks)
    rows = eng.perm_generate(masks, margins, N, P, base, 5).cpu().numpy().view(np.uint32)
    tiles = eng.perm_generate_tiles(masks, margins, N, P, base, 5).cpu().numpy().view(np.uint32)
    lanes, stride, gpw, classes, _piece = eng.list_params(N)
    RS = stride // 4
    tperm = lanes * 32
    ntiles = -(-P // tperm)
    tw = int(eng.lib.scoary_list_tile_words(N))
    tiles = tiles.reshape(T, ntiles, tw)[:, :, :(N + 1) * RS].reshape(T, ntiles, N + 1, RS)
    bits = np.unpackbits(rows.view(np.uint8).reshape(T, P, -1), axis=2, bitorder="little")[:, :, :N]
    for t in range(T):
        for tile in range(ntiles):
            tb_ = np.unpackbits(np.ascontiguousarray(tiles[t, tile, :, :lanes]).view(np.uint8),
                                axis=1, bitorder="little")            # (N+1, tile perms)
            assert not tb_[N].any()
            lo, hi = tile * tperm, min(P, tile * tperm + tperm)
            assert np.array_equal(tb_[:N, :hi - lo], bits[t, lo:hi].T)
            assert not tb_[:N, hi - lo:].any()


def test_capacity_config_shard_vs_oracle_subsample(eng, orc):
    """BASELINE configs[4] ("HBM-capacity stress", 1M x 10000 x 50 over 8 GPUs):
    one GPU's row length and trait count at a reduced gene / permutation count
    (the per-GPU shard is 125k genes; 20k here keep the host-side generation
    short).  Exercises the chunked dense kernel (N > 5119), 50 traits, int64
    indexing; a gene subsample is compared with the oracle bit for bit."""
    from scoary_amd import synth
    rng = np.random.default_rng(20260904)
    G, N, T, P = 20000, 10000, 50, 96
    genes = synth.make_genes(G, N, rng, core_frac=0.05)
    traits = synth.make_traits(T, N, rng, missing_traits=(8, 9, 33))
    tb, mb = _bits(eng, traits)
    from scoary_amd.engine import pack_bits_rows
    gm = eng.pack_dense(genes)
    res = eng.associate(gm, eng.vecrows(tb, N), eng.vecrows(mb, N), permutations=P, seed=11,
                        use_lists=False)                    # chunked dense kernel
    eng.build_lists(gm)
    res_l = eng.associate(gm, eng.vecrows(tb, N), eng.vecrows(mb, N), permutations=P, seed=11,
                          use_lists=True)                   # 4-lane list kernel
    assert np.array_equal(res_l["r"].cpu().numpy(), res["r"].cpu().numpy())
    counts = res["counts"].cpu().numpy()
    r = res["r"].cpu().numpy().view(np.uint32)
    p = res["p"].cpu().numpy()
    nval = (traits != 2).sum(1)
    assert np.array_equal(counts.sum(2), np.broadcast_to(nval[:, None], (T, G)))
    assert r.max() <= P
    sub = np.arange(0, G, 331)
    gb = orc.pack_rows(genes[sub])
    want_c = orc.counts_packed(gb, tb, mb).transpose(1, 0, 2)
    assert np.array_equal(counts[:, sub], want_c)
    _, want_p = orc.fisher_many(np.ascontiguousarray(want_c).reshape(-1, 4))
    assert np.max(np.abs(p[:, sub].ravel() - want_p)) < P_TOL
    assert np.array_equal(r[:, sub], orc.permute_r(gb, tb, mb, N, P, 11).T)


def test_c_abi_error_codes(eng):
    """Bad arguments come back as negative status + message, never a crash."""
    import ctypes
    import torch
    lib, h = eng.lib, eng.h
    null = ctypes.c_void_p()
    buf = torch.zeros(1024, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.scoary_counts(h, null, p, p, 1, 1, 1, p, p, null) == -1
    assert b"scoary_counts" in lib.scoary_last_error(h)
    assert lib.scoary_fisher(h, p, 0, p, p, null, null) == -1
    assert lib.scoary_fisher_lists(h, p, 1, 1, p, p, p, p, null, null, null) == -1        # no d_lcrit
    assert lib.scoary_permute_lists(h, p, p, 0, p, p, p, p, null, null, p, p, 4, 1, 100, 10, p, 1, null) == -1
    assert lib.scoary_permute(h, p, p, p, 1, 70000, 10, 10, p, null) == -3          # T > 65535
    assert lib.scoary_perm_generate(h, p, p, 1, 10, 2**33, 0, 0, 1, p, null) == -3   # index >= 2^32
    nmax = int(lib.scoary_perm_max_isolates())
    assert nmax >= 600_000                                                             # one permutation per LDS row
    assert lib.scoary_perm_generate(h, p, p, 1, nmax + 1, 1, 0, 0, 1, p, null) == -3
    assert lib.scoary_perm_generate_tiles(h, p, p, 1, 100, 64, 40, 0, 1, p, null) == -1   # tiles start at a multiple of 32
    assert lib.scoary_perm_generate_tiles_range(h, p, p, 2, 100, 600, 0, 0, 1, 3, 2, p, null) == -1   # 2 x 2 tiles: range past the end
    assert lib.scoary_permute_lists(h, p, p, 0, p, p, p, p, p, null, p, p, 4, 1, 131071, 10, p, 1, null) == -3
    assert b"LDS" in lib.scoary_last_error(h)
    assert lib.scoary_tree_pairs(h, p, 3, 40, p, p, 1, 1, 2, p, null) == -3          # stack_depth > 32
    assert lib.scoary_counts(null, p, p, p, 1, 1, 1, p, p, null) == -1
    out = ctypes.c_void_p()
    assert lib.scoary_create(99, ctypes.byref(out)) == -4 and not out.value
    params = (ctypes.c_int64 * 5)()
    assert lib.scoary_list_params(2000, params) == 0 and list(params) == [16, 64, 16, 4, 16]
    assert lib.scoary_list_params(5000, params) == 0 and list(params) == [8, 32, 32, 8, 8]
    assert lib.scoary_list_params(5120, params) == 0 and list(params) == [4, 16, 64, 16, 4]
    assert lib.scoary_list_params(10240, params) == 0 and list(params) == [2, 8, 64, 32, 4]
    assert lib.scoary_list_params(20480, params) == 0 and list(params) == [2, 8, 64, 32, 8]   # 2 segments: 16-bit entries, 8 per vector
    assert lib.scoary_list_params(131071, params) == -3 and params[0] == 0
    assert lib.scoary_list_max_isolates() == 131070
    assert [lib.scoary_list_segments(n) for n in (1, 20479, 20480, 40704, 40705, 122112, 122113, 131070, 131071)] \
        == [1, 1, 2, 2, 3, 6, 7, 7, 0]


# ------------------------------------------- spec S6: device list builder -----
@pytest.mark.parametrize("G,N", [(1, 1), (5, 31), (203, 333), (1000, 500), (3000, 2000), (700, 2559),
                                 (900, 2560), (650, 5000), (300, 5120), (257, 10000), (130, 10240),
                                 (100, 20479)])
def test_device_list_builder_equals_host_builder(eng, G, N):
    """scoary_lists_plan + scoary_lists_fill (device, product path) write the same
    arrays -- order, start, ngroups, flipped and every index entry -- as the host
    builder scoary_lists_build (the checker; an independent implementation of spec
    S6), for all four tile widths, ties in the length sort, empty and full genes and
    a ragged last wave group (the segmented lists of N > 20479 are checked position by position
    in test_segmented_list_path_vs_dense_and_oracle)."""
    from scoary_amd import io_native
    from scoary_amd.engine import pack_bits_rows
    rng = np.random.default_rng(G * 31 + N)
    genes = (rng.random((G, N)) < rng.uniform(0.0, 1.0, (G, 1))).astype(np.uint8)
    if G > 4:
        genes[0] = 0
        genes[1] = 1
        genes[3] = genes[2]                      # equal lengths: the sort must be stable
        genes[G - 1] = genes[2]
    gm = eng.pack_dense(genes)
    L = eng.build_lists(gm)
    lanes, stride, gpw, classes, piece = eng.list_params(N)
    H = io_native.build_lists(pack_bits_rows(genes), N, stride, gpw, classes, piece)
    assert L.entries == H["entries"]
    assert np.array_equal(L.order.cpu().numpy(), H["order"])
    assert np.array_equal(L.flipped.cpu().numpy(), H["flipped"])
    assert np.array_equal(L.start.cpu().numpy(), H["start"])
    assert np.array_equal(L.ngroups.cpu().numpy(), H["ngroups"])
    got = L.idx.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:L.entries], H["idx"][:L.entries])
    assert not got[L.entries:].any()             # slack entries are zero


def test_device_list_builder_baseline_shapes(eng):
    """Device-built lists == host-built lists at the BASELINE list shapes: cfg2
    (10 000 x 500), cfg3 (50 000 x 2000, 5 % core genes) and a cfg4 slice (rare
    variants, N = 5000)."""
    from scoary_amd import io_native, synth
    from scoary_amd.engine import pack_bits_rows
    for name, G in (("cfg2", None), ("cfg3", None), ("cfg4", 30000)):
        genes, _traits, _P, _seed = synth.make_config(name, G=G)
        N = genes.shape[1]
        gm = eng.pack_dense(genes)
        L = eng.build_lists(gm)
        lanes, stride, gpw, classes, piece = eng.list_params(N)
        H = io_native.build_lists(pack_bits_rows(genes), N, stride, gpw, classes, piece)
        assert L.entries == H["entries"], name
        assert np.array_equal(L.order.cpu().numpy(), H["order"]), name
        assert np.array_equal(L.start.cpu().numpy(), H["start"]), name
        assert np.array_equal(L.idx.cpu().numpy().view(np.uint32)[:L.entries],
                              H["idx"][:L.entries]), name


# ------------------------------------------------ workspace / hipGraph -----
@pytest.mark.parametrize("use_lists", [True, False])
def test_workspace_and_graph_replay_equal_eager(eng, orc, use_lists):
    """A step through a reusable workspace, and the same step captured into a
    hipGraph (scoary_graph_*) and replayed, give the results of the eager path and
    of the oracle; replays are idempotent (r is re-zeroed inside the graph)."""
    import torch
    rng = np.random.default_rng(77)
    G, N, T, P = 900, 400, 2, 700
    genes, traits = _random_case(rng, G, N, T)
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    eng.build_lists(gm)
    eager = eng.associate(gm, trv, mkv, permutations=P, seed=3, use_lists=use_lists)
    want_r = eager["r"].cpu().numpy().copy()
    want_p = eager["p"].cpu().numpy().copy()
    ws = eng.workspace(gm, T, P, use_lists=use_lists)
    for _ in range(2):
        res = eng.associate(gm, trv, mkv, permutations=P, seed=3, use_lists=use_lists, workspace=ws)
        assert np.array_equal(res["r"].cpu().numpy(), want_r)
    graph, res = eng.capture(gm, trv, mkv, P, 3, ws, use_lists=use_lists)
    for _ in range(3):
        ws.r.fill_(-1)
        ws.p.fill_(0.0)
        graph.launch()
        torch.cuda.synchronize()
        assert np.array_equal(res["r"].cpu().numpy(), want_r)
        assert np.array_equal(res["p"].cpu().numpy(), want_p)
    graph.close()
    assert np.array_equal(want_r.view(np.uint32),
                          orc.permute_r(orc.pack_rows(genes), tb, mb, N, P, 3).T)
    with pytest.raises(ValueError):
        eng.associate(gm, trv, mkv, permutations=P + 1, seed=3, use_lists=use_lists, workspace=ws)


@pytest.mark.parametrize("use_lists", [True, False], ids=["lists", "dense"])
def test_launch_bound_steps_replay_a_graph_by_themselves(eng, orc, use_lists, monkeypatch):
    """Round 4: with a workspace AND a trait plan -- every buffer persistent --
    associate() records a launch-bound step (auto_graph_eligible: < 5e8 tests) into a hipGraph on
    its second call and replays it from the third on.  Results equal the eager step's and the
    oracle's on every call; other buffers, another seed or graph=False fall back to eager; per-kernel
    timing and SCOARY_AUTO_GRAPH=0 switch it off; a step too large is never recorded."""
    import torch
    rng = np.random.default_rng(78)
    G, N, T, P = 700, 300, 3, 300
    genes, traits = _random_case(rng, G, N, T)
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    eng.build_lists(gm)
    plan = eng.trait_plan(trv, mkv, N)
    want = orc.permute_r(orc.pack_rows(genes), tb, mb, N, P, 5).T
    ws = eng.workspace(gm, T, P, use_lists=use_lists)
    assert eng.auto_graph_eligible(gm, T, P) and ws.auto is None
    for call in range(5):
        ws.r.fill_(-1)
        res = eng.associate(gm, trv, mkv, permutations=P, seed=5, use_lists=use_lists, workspace=ws, plan=plan)
        torch.cuda.synchronize()
        assert np.array_equal(res["r"].cpu().numpy().view(np.uint32), want), call
        assert (ws.auto["graph"] is not None) == (call >= 1)          # recorded on the second call
    g1 = ws.auto["graph"]
    res = eng.associate(gm, trv, mkv, permutations=P, seed=6, use_lists=use_lists, workspace=ws, plan=plan)
    assert ws.auto["graph"] is None and g1.graph is None               # another seed: old graph closed, eager again
    assert np.array_equal(res["r"].cpu().numpy().view(np.uint32), orc.permute_r(orc.pack_rows(genes), tb, mb, N, P, 6).T)
    res = eng.associate(gm, trv, mkv, permutations=P, seed=6, use_lists=use_lists, workspace=ws, plan=plan, graph=False)
    assert ws.auto["graph"] is None                                    # graph=False never records
    eng.set_timing(True)                                               # per-kernel events: eager
    try:
        eng.associate(gm, trv, mkv, permutations=P, seed=6, use_lists=use_lists, workspace=ws, plan=plan)
        assert ws.auto["graph"] is None and eng.kernel_ms("k_counts") > 0
    finally:
        eng.set_timing(False)
    monkeypatch.setenv("SCOARY_AUTO_GRAPH", "0")
    assert not eng.auto_graph_eligible(gm, T, P)
    monkeypatch.delenv("SCOARY_AUTO_GRAPH")
    assert not eng.auto_graph_eligible(gm, 1000, 1000)                 # 7e8 tests: not launch-bound
    # without a plan the step recomputes it and stays eager (nothing persistent to replay against)
    ws2 = eng.workspace(gm, T, P, use_lists=use_lists)
    for _ in range(3):
        res = eng.associate(gm, trv, mkv, permutations=P, seed=5, use_lists=use_lists, workspace=ws2)
    assert ws2.auto is None and np.array_equal(res["r"].cpu().numpy().view(np.uint32), want)


# ------------------------------ opt-in early abort on the Fisher statistic -----
# tiled row size (quads) of the early-abort cases: k_permute_seq walks a row in chunks of the largest of 8 / 4 / 2 / 1
# quads that divides it.  The (70, N, 2, 64) cases are one small shape per chunk width: 8, 4, 2 and 1
SEQ_ROW_QUADS = {90: 1, 100: 1, 400: 4, 700: 6, 900: 8, 1000: 8, 2100: 20, 7000: 56}


@pytest.mark.parametrize("G,N,T,P", [(120, 90, 2, 200), (70, 700, 1, 333), (40, 2100, 2, 130), (64, 1000, 1, 120),
                                     (30, 7000, 1, 70)]
                         + [(70, N, 2, 64) for N in (900, 400, 700, 100)])
def test_permute_sequential_early_abort_vs_oracle(eng, orc, G, N, T, P):
    """--permute-early-abort (scoary_permute_seq): the reference's sequential estimator
    (scoary/methods.py:1348-1365) applied to the Fisher statistic.  The oracle leg states
    it independently: per permutation the Fisher p of the permuted table (spec-S4 labels)
    against the observed p, then the reference's loop (oracle.empirical_p_with_abort, which
    calls binom.cdf per step like the reference).  r, the stopping point and the estimate
    agree for every (gene, trait); batching the permutations changes nothing."""
    from scoary_amd import tree as T_
    assert eng.quads(N) == SEQ_ROW_QUADS[N]             # which chunk width the shape reaches
    rng = np.random.default_rng(G + N + P)
    genes, traits = _random_case(rng, G, N, T)
    genes[3] = (rng.random(N) < 0.5).astype(np.uint8)
    traits[0] = np.where(rng.random(N) < 0.6, genes[3], traits[0])          # one strong association
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    seed = 31 + P
    res = eng.associate(gm, trv, mkv, permutations=0)
    crit = eng.fisher(res["counts"], want_crit=True)[2]
    thr = T_._abort_thresholds(P)
    r, nstop = eng.permute_sequential(gm, mkv, res["margins"], crit, P, seed, thr)
    r = r.cpu().numpy().view(np.uint32)
    nstop = nstop.cpu().numpy().view(np.uint32)
    got = (r + 1.0) / (np.where(nstop > 0, nstop, P) + 1.0)
    counts = res["counts"].cpu().numpy()
    p_obs = res["p"].cpu().numpy()
    stopped = 0
    for t in range(T):
        npos = int((traits[t] == 1).sum())
        labels = np.stack([np.unpackbits(orc.perm_labels(seed, t, pi, mb[t], npos, N).view(np.uint8),
                                         bitorder="little")[:N] for pi in range(P)])      # (P, N)
        valid = traits[t] != 2
        a = labels[:, valid].astype(np.int64) @ genes[:, valid].T.astype(np.int64)        # (P, G)
        for g in range(G):
            c = counts[t, g]
            if c[0] + c[2] == 0 or c[1] + c[3] == 0:        # never tested: every permutation "reaches" it
                flags = np.ones(P, dtype=bool)
            else:
                n1, gm_ = c[0] + c[1], c[0] + c[2]
                tab = np.stack([a[:, g], n1 - a[:, g], gm_ - a[:, g],
                                c.sum() - n1 - gm_ + a[:, g]], axis=1).astype(np.int32)
                _, pp = orc.fisher_many(tab)
                flags = pp <= p_obs[t, g] * (1 + 1e-7)
            want = orc.empirical_p_with_abort(flags)
            assert got[t, g] == want, (t, g, got[t, g], want, nstop[t, g])
            stopped += nstop[t, g] > 0
    assert 0 < stopped < G * T          # both branches of the estimator occurred
    # a one-batch run equals a many-batch run (state carried in d_r / d_nstop)
    small = eng.perm_batch
    try:
        eng.perm_batch = lambda T__, N__, P__, budget_bytes=0: 37
        r2, n2 = eng.permute_sequential(gm, mkv, res["margins"], crit, P, seed, thr)
    finally:
        eng.perm_batch = small
    assert np.array_equal(r2.cpu().numpy().view(np.uint32), r)
    assert np.array_equal(n2.cpu().numpy().view(np.uint32), nstop)


def test_fisher_on_the_near_tie_census_tables(eng):
    """k_fisher on the closest non-equal weight pairs there are (tests/golden/near_ties.json,
    exhaustive census with exact-rational p-values; 34 of the pairs are closer than 1e-10
    without being equal): p equals the exact p under spec S3's rule -- SciPy's 1 + 1e-14,
    decided in double-double arithmetic when the fp64 weights agree to 1e-9 -- to 1e-12, and
    the rejection regions separate the two points of every pair the way the exact rule does."""
    import torch
    with open(os.path.join(GOLDEN, "near_ties.json")) as f:
        d = json.load(f)
    tabs, want = [], []
    for c in d["cases"]:
        for t in c["tables"]:
            tabs.append([t["a"], t["b"], t["c"], t["d"]])
            want.append(t["p_tie_1e-14"])
    assert len(tabs) == 104
    p, _, crit = eng.fisher(torch.tensor(tabs, dtype=torch.int32, device="cuda"), want_crit=True)
    assert np.max(np.abs(p.cpu().numpy() - np.array(want))) < P_TOL
    crit = crit.cpu().numpy().view(np.uint32)
    k = 0
    for c in d["cases"]:
        for t in c["tables"]:
            base, span = int(crit[k, 0]), int(crit[k, 1])
            other = c["y"] if t["a"] == c["x"] else c["x"]
            bigger_other = (c["rel_gap"] > 0) == (other == c["y"])     # is the partner's weight the larger one?
            in_region = not (base <= other < base + span)
            assert in_region == (not bigger_other), (c, t, base, span)
            k += 1


def test_pack_records_kernel_equals_the_host_side_packing(eng):
    """scoary_pack_records (one kernel) writes the same [T, G, 10] int32 records as
    scoary_amd.dist.pack_records (tensor ops; what the gloo tests use) -- bit patterns of p /
    odds preserved, r / nstop optional -- and unpack_records inverts it."""
    import torch
    from scoary_amd import dist as sd
    rng = np.random.default_rng(3)
    genes, traits = _random_case(rng, 700, 300, 3)
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    res = eng.associate(gm, eng.vecrows(tb, 300), eng.vecrows(mb, 300), permutations=100, seed=1)
    nstop = torch.arange(3 * 700, dtype=torch.int32, device="cuda").view(3, 700)
    got = eng.pack_records(res, nstop=nstop)
    want = sd.pack_records(res["counts"], res["p"], res["odds"], res["r"], nstop)
    assert torch.equal(got, want)
    d = sd.unpack_records(got)
    assert torch.equal(d["p"], res["p"]) or torch.equal(d["p"].isnan(), res["p"].isnan())
    assert torch.equal(d["r"], res["r"]) and torch.equal(d["nstop"], nstop)
    none = eng.pack_records({"counts": res["counts"], "p": res["p"], "odds": res["odds"], "r": None})
    assert torch.equal(none, sd.pack_records(res["counts"], res["p"], res["odds"], None))


@pytest.mark.parametrize("G,N,T,P", [(500, 600, 2, 1700), (90, 21_000, 2, 1100)],
                         ids=["one-tile", "segmented-tiles"])
def test_list_path_in_batches_equals_one_shot_and_oracle(eng, orc, monkeypatch, G, N, T, P):
    """The list-driven path with the permutations split into batches of label tiles (what a
    cfg5-size run does to bound the tile and per-tile-count buffers): r accumulates over the
    batches, permutation indices stay global -- identical to the one-batch run and the oracle,
    also through the segmented kernel of N > 20479; list_batch keeps the 16-bit count scratch
    of a cfg5 shard under 4 GB."""
    rng = np.random.default_rng(41)
    genes, traits = _random_case(rng, G, N, T)
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    eng.build_lists(gm)
    one = eng.associate(gm, trv, mkv, permutations=P, seed=9, use_lists=True)["r"].cpu().numpy()
    monkeypatch.setattr(eng, "list_batch", lambda *a, **k: 512)
    many = eng.associate(gm, trv, mkv, permutations=P, seed=9, use_lists=True)["r"].cpu().numpy()
    monkeypatch.undo()
    assert np.array_equal(one, many)
    assert np.array_equal(one.view(np.uint32), orc.permute_r(orc.pack_rows(genes), tb, mb, N, P, 9).T)
    b = eng.list_batch(50, 10000, 100000, 125000)
    assert b % 512 == 0 and 2 * 50 * 125064 * (b // 128) <= 4 << 30 and b >= 32768
    assert eng.list_batch(10, 2000, 10000, 50000) == 10240          # the headline config: one batch


@pytest.mark.parametrize("N,T", [(333, 3), (2600, 2), (5200, 1)])
def test_fisher_in_slot_order_and_fused_regions(eng, N, T):
    from scoary_amd.engine import pack_bits_rows
    """scoary_fisher_lists: the tables visited in list-slot order give bit-identical p /
    odds / regions to scoary_fisher (a table's result does not depend on its neighbours),
    and the slot-order regions it emits drive scoary_permute_lists to the same r as the
    gene-order regions converted by k_lists_crit; accumulate = 0 overwrites r."""
    import torch
    from scoary_amd import synth
    rng = np.random.default_rng(N)
    G, P, seed = 3000, 700, 5
    genes = synth.make_genes(G, N, rng, core_frac=0.03)
    traits = synth.make_traits(T, N, rng, missing_traits=(0,), missing_frac=0.05)
    gm = eng.pack_dense(genes)
    eng.build_lists(gm)
    trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
    mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
    counts, margins = eng.counts(gm, trv, mkv)
    p0, o0, c0 = eng.fisher(counts)
    p1, o1, c1, lc = eng.fisher(counts, lists=gm.lists)
    assert torch.equal(p0.view(torch.int64), p1.view(torch.int64))
    assert torch.equal(o0.view(torch.int64), o1.view(torch.int64))
    assert torch.equal(c0, c1)
    # the conversion rule, restated on the host
    order = gm.lists.order.cpu().numpy()
    fl = gm.lists.flipped.cpu().numpy().astype(bool)[order]
    c = c0.cpu().numpy().view(np.uint32)[:, order, :].astype(np.int64)
    npos = margins.cpu().numpy()[:, 0].astype(np.int64)[:, None]
    lo = np.where(fl[None, :], npos - c[..., 0] - c[..., 1] + 1, c[..., 0])
    hi = np.where(fl[None, :], npos - c[..., 0] + 1, c[..., 0] + c[..., 1])
    lo, hi = np.where(c[..., 1] == 0, 0, lo), np.where(c[..., 1] == 0, 0, hi)
    got = lc.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(got[..., 0], lo) and np.array_equal(got[..., 1], hi)
    tiles = eng.perm_generate_tiles(mkv, margins, N, P, 0, seed)
    r0 = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    eng.permute_lists(gm, tiles, c0, margins, P, r0)
    r1 = torch.full((T, G), 12345, dtype=torch.int32, device=eng.device)
    eng.permute_lists(gm, tiles, None, margins, P, r1, lcrit=lc, accumulate=False)
    assert torch.equal(r0, r1)
    eng.permute_lists(gm, tiles, None, margins, P, r1, lcrit=lc, accumulate=True)
    assert torch.equal(2 * r0, r1)
    # and the whole step, against the dense kernels
    res = eng.associate(gm, trv, mkv, permutations=P, seed=seed)
    ref = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=False)
    assert torch.equal(res["r"], ref["r"]) and torch.equal(res["crit"], ref["crit"])


def test_fisher_symmetric_margins_and_large_n(eng, orc):
    """Tables with a symmetric margin pair (n1 == n2, or n == N - n) have an exact mirror
    tie for every a: k_fisher settles those without arithmetic (x == a, x == n - a,
    x == n1 - a).  p against the oracle (which compares big integers), the acceptance
    interval symmetric about the centre, up to the largest N the list path takes; plus
    unconstrained tables at large N."""
    import torch
    rng = np.random.default_rng(77)
    tabs, kinds = [], []
    for N in (10, 64, 500, 2000, 5000, 20000, 40958):
        for _ in range(60):
            kind = int(rng.integers(0, 3))
            if kind == 0:                                   # n1 == n2
                n1 = N // 2; Nn = 2 * n1
                n = int(rng.integers(1, Nn))
            elif kind == 1:                                 # n == N - n
                n = N // 2; Nn = 2 * n
                n1 = int(rng.integers(1, Nn))
            else:
                Nn = N; n1 = int(rng.integers(1, N)); n = int(rng.integers(1, N))
            n2 = Nn - n1
            lo, hi = max(0, n - n2), min(n, n1)
            mode = (n + 1) * (n1 + 1) // (Nn + 2)
            sd = max(1.0, (n * n1 / Nn * n2 / Nn * (Nn - n) / max(Nn - 1, 1)) ** 0.5)
            a = int(np.clip(round(mode + rng.normal() * 2.5 * sd), lo, hi))
            tabs.append((a, n1 - a, n - a, n2 - n + a)); kinds.append(kind)
    tabs = np.array(tabs, dtype=np.int32)
    assert tabs.min() >= 0
    p, odds, crit = eng.fisher(torch.from_numpy(tabs).cuda())
    p = p.cpu().numpy()
    crit = crit.cpu().numpy().view(np.uint32).astype(np.int64)
    _, o_p = orc.fisher_many(tabs)
    assert np.max(np.abs(p - o_p)) < P_TOL
    ok = o_p > 1e-280
    assert np.max(np.abs(p[ok] - o_p[ok]) / o_p[ok]) < 1e-10
    checked = 0
    for (a, b, c, d), kind, (base, span) in zip(tabs.tolist(), kinds, crit.tolist()):
        if kind == 2 or span == 0:
            continue
        centre2 = (a + c) if kind == 0 else (a + b)         # x -> n - x  or  x -> n1 - x
        assert base + (base + span - 1) == centre2, (a, b, c, d, base, span)
        checked += 1
    assert checked > 150


def test_index_lists_over_budget_fall_back_to_the_dense_kernels(eng, orc, caplog, monkeypatch):
    """the list path now serves every N <= 131 070, and a wide, dense matrix can ask
    for a very large index array.  scoary_lists_plan returns the size before anything is
    allocated: over the budget build_lists raises ListMemoryError (no allocation, genes.lists
    stays None) and the command line's _associate logs it and keeps the dense kernels -- same
    results."""
    import logging
    from scoary_amd import methods as M
    from scoary_amd.engine import ListMemoryError, pack_bits_rows
    rng = np.random.default_rng(620)
    G, N, T, P = 300, 700, 2, 64
    genes, traits = _random_case(rng, G, N, T)
    gm = eng.pack_dense(genes)
    with pytest.raises(ListMemoryError):
        eng.build_lists(gm, budget_bytes=1000)
    assert gm.lists is None
    assert eng.build_lists(gm, budget_bytes=1 << 30) is gm.lists and gm.lists is not None
    table = M.GeneTable(["g%d" % i for i in range(G)], [""] * G, [""] * G,
                        ["s%d" % i for i in range(N)], pack_bits_rows(genes))
    monkeypatch.setenv("SCOARY_LIST_BUDGET_MB", "0.001")
    M._ENGINE = eng
    try:
        with caplog.at_level(logging.INFO, logger=M.log.name):
            out = M._associate(table, traits, permutations=P, seed=5)
    finally:
        M._ENGINE = None
    assert any("index lists not built" in r.getMessage() for r in caplog.records)
    tb, mb = _bits(eng, traits)
    gb = orc.pack_rows(genes)
    assert np.array_equal(out["counts"], orc.counts_packed(gb, tb, mb).transpose(1, 0, 2))
    assert np.array_equal(out["r"], orc.permute_r(gb, tb, mb, N, P, 5).T)


def _large_n_tables(rng, sizes, per_size):
    """Random and symmetric-margin 2x2 tables (a, b, c, d) at large population sizes, observed
    count a few standard deviations around the mode (so p is neither 0 nor 1)."""
    tabs = []
    for N in sizes:
        for i in range(per_size):
            kind = i % 4
            if kind == 0:                                   # n1 == n2
                n1 = N // 2; Nn = 2 * n1
                n = int(rng.integers(1, Nn))
            elif kind == 1:                                 # n == N - n
                n = N // 2; Nn = 2 * n
                n1 = int(rng.integers(1, Nn))
            elif kind == 2:                                 # a rare gene or a rare trait
                Nn = N; n1 = int(rng.integers(1, N)); n = int(rng.integers(1, 400))
            else:
                Nn = N; n1 = int(rng.integers(1, N)); n = int(rng.integers(1, N))
            n2 = Nn - n1
            lo, hi = max(0, n - n2), min(n, n1)
            mode = (n + 1) * (n1 + 1) // (Nn + 2)
            sd = max(1.0, (n * n1 / Nn * n2 / Nn * (Nn - n) / max(Nn - 1, 1)) ** 0.5)
            a = int(np.clip(round(mode + rng.normal() * 2.5 * sd), lo, hi))
            tabs.append((a, n1 - a, n - a, n2 - n + a))
    return np.array(tabs, dtype=np.int32)


def test_fisher_where_the_segmented_list_path_goes(eng, orc):
    """k_fisher for 40 958 < N <= 131 070: since round 3 the list path --
    and with it scoary_fisher_lists' p, odds and acceptance intervals -- serves matrices this wide,
    and the direct checks stopped at 40 958.  Random, rare-margin and symmetric-margin tables at
    N = 50 000, 90 001 and 131 070 against the oracle, whose own p is pinned to EXACT rational
    arithmetic at these sizes by tests/test_oracle_golden.py::test_oracle_fisher_vs_exact_rationals_large_n
    (SciPy 1.15.3 itself is up to 6e-12 off the exact value up here, so the oracle is the
    yardstick, not SciPy).  Reference call site: scoary/methods.py:854."""
    import torch
    rng = np.random.default_rng(131070)
    tabs = _large_n_tables(rng, (50_000, 90_001, 131_070), 80)
    tabs = np.concatenate([tabs, np.array([[5582, 3263, 70693, 40462]], dtype=np.int32)])   # N = 120 000
    assert tabs.min() >= 0 and tabs.sum(1).max() <= 131_070
    p, odds, crit = eng.fisher(torch.from_numpy(tabs).cuda())
    p, odds = p.cpu().numpy(), odds.cpu().numpy()
    crit = crit.cpu().numpy().view(np.uint32).astype(np.int64)
    o_odds, o_p = orc.fisher_many(tabs)
    assert np.max(np.abs(p - o_p)) < P_TOL
    ok = o_p > 1e-280
    assert ok.sum() > 200 and np.max(np.abs(p[ok] - o_p[ok]) / o_p[ok]) < 1e-10
    fin = np.isfinite(o_odds)
    assert np.array_equal(fin, np.isfinite(odds)) and np.allclose(odds[fin], o_odds[fin], rtol=1e-15, atol=0)
    # the exact value of the N = 120 000 table (computed in rationals; SciPy says ...243636)
    assert abs(p[-1] - 0.3584981573183696) < 1e-13
    # the acceptance interval contains the observed count's complement: a is on its edge or outside
    a = tabs[:, 0].astype(np.int64)
    inside = (a >= crit[:, 0]) & (a < crit[:, 0] + crit[:, 1])
    assert not inside.any()                                  # p_obs <= p_obs: the observed table is in the region


def test_more_isolates_than_the_list_kernel_takes(eng, orc, caplog):
    """N > 131 070 (the list counts would need a 17th counter plane): the list builder refuses, associate() and the command line's
    _associate fall back to the dense kernels -- and say so in the log (VERDICT round 2,
    item 8) -- with results equal to the oracle's.  No BASELINE config is this wide."""
    import logging
    from scoary_amd import methods as M
    from scoary_amd.engine import pack_bits_rows
    rng = np.random.default_rng(50)
    G, N, T, P = 100, 131_071, 2, 40
    genes, traits = _random_case(rng, G, N, T)
    assert not eng.lists_supported(N) and eng.lists_supported(N - 1)
    assert eng.lib.scoary_list_segments(N) == 0 and eng.lib.scoary_list_segments(N - 1) == 7
    gm = eng.pack_dense(genes)
    with pytest.raises(ValueError):
        eng.build_lists(gm)
    table = M.GeneTable(["g%d" % i for i in range(G)], [""] * G, [""] * G,
                        ["s%d" % i for i in range(N)], pack_bits_rows(genes))
    M._ENGINE = eng
    try:
        with caplog.at_level(logging.INFO, logger=M.log.name):
            out = M._associate(table, traits, permutations=P, seed=77)
    finally:
        M._ENGINE = None
    assert any("dense permutation kernels" in r.getMessage() for r in caplog.records)
    tb, mb = _bits(eng, traits)
    gb = orc.pack_rows(genes)
    assert np.array_equal(out["counts"], orc.counts_packed(gb, tb, mb).transpose(1, 0, 2))
    assert np.array_equal(out["r"], orc.permute_r(gb, tb, mb, N, P, 77).T)


@pytest.mark.parametrize("G,N,T,P", [(150, 20_480, 2, 70), (333, 50_000, 2, 133), (70, 90_001, 1, 100),
                                     (64, 131_070, 1, 64)])
def test_segmented_list_path_vs_dense_and_oracle(eng, orc, G, N, T, P):
    """20 479 < N <= 131 070 (round 3; one-dword tiles up to 40 959 and the dense kernels beyond
    it before): the isolates are cut into 2 ... 7 segments of 20 352, a block loads its
    64-permutation tile one segment at a time, every gene has one sub-list per segment and the
    counter planes live across the reloads (k_permute_seglists).  Checked: (1) the label tiles
    hold the rows of k_perm_generate, every segment with its own zero row; (2) every sub-list
    holds exactly the gene's minority positions of that segment, as 16-bit row indices in
    grid-compaction order, zero-row padded; (3) r is bit-identical to the dense kernels' and to
    the oracle's."""
    rng = np.random.default_rng(G + N)
    genes, traits = _random_case(rng, G, N, T)
    genes[5] = (rng.random(N) < 0.0005)                   # sub-lists that are empty in a segment
    genes[6, :20_352] = 0
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    S = int(eng.lib.scoary_list_segments(N))
    SEG, STRIDE = 20_352, 40_708
    assert S == -(-N // SEG) and eng.list_params(N) == (2, 8, 64, 32, 8)
    # (1) tiles: [T][tiles][S][STRIDE dwords], row r of segment s = dwords 2r, 2r + 1
    _, margins = eng.counts(gm, trv, mkv)
    rows = eng.perm_generate(mkv, margins, N, P, 32, 17).cpu().numpy().view(np.uint32)
    tiles = eng.perm_generate_tiles(mkv, margins, N, P, 32, 17).cpu().numpy().view(np.uint32)
    ntiles = -(-P // 64)
    assert int(eng.lib.scoary_list_tile_words(N)) == S * STRIDE
    tiles = tiles.reshape(T, ntiles, S, STRIDE)
    bits = np.unpackbits(rows.view(np.uint8).reshape(T, P, -1), axis=2, bitorder="little")[:, :, :N]
    for s in range(S):
        n_s = min(SEG, N - s * SEG)
        tb_ = np.unpackbits(np.ascontiguousarray(tiles[:, :, s, :2 * (n_s + 1)]).view(np.uint8)
                            .reshape(T, ntiles, n_s + 1, 8), axis=3, bitorder="little")
        assert not tb_[:, :, n_s].any()                   # the segment's zero row
        for tile in range(ntiles):
            lo, hi = tile * 64, min(P, tile * 64 + 64)
            assert np.array_equal(tb_[:, tile, :n_s, :hi - lo],
                                  bits[:, lo:hi, s * SEG:s * SEG + n_s].transpose(0, 2, 1))
            assert not tb_[:, tile, :n_s, hi - lo:].any()
    # (2) lists
    L = eng.build_lists(gm)
    # 16-bit entries (round 4): the row index inside the segment, eight per lane and 16-byte index
    # vector; start counts 128-byte units = 64 entries; L.entries counts 32-bit words
    idx = L.idx.cpu().numpy().view(np.uint16)
    start = L.start.cpu().numpy().astype(np.int64).reshape(S, G) * 64
    nhalf = L.ngroups.cpu().numpy().astype(np.int64).reshape(S, G)
    order, flipped = L.order.cpu().numpy(), L.flipped.cpu().numpy()
    ones = genes.sum(1, dtype=np.int64)
    assert np.array_equal(flipped.astype(bool), 2 * ones > N)
    lens = np.minimum(ones, N - ones)
    assert np.array_equal(np.sort(order), np.arange(G)) and np.all(np.diff(lens[order]) <= 0)
    for k in range(G):
        q, j = divmod(k, 64)
        g = order[k]
        minority = genes[g] == (0 if flipped[g] else 1)
        for s in range(S):
            n_s = min(SEG, N - s * SEG)
            n = np.arange(nhalf[s, q * 64] * 16)
            at = start[s, q * 64] + ((n // 8) * 64 + j) * 8 + n % 8
            vals = idx[at]
            want = np.flatnonzero(minority[s * SEG:s * SEG + n_s])
            assert np.array_equal(np.sort(vals[:len(want)]), want)
            assert np.all(vals[len(want):] == n_s)
            assert nhalf[s, k] == nhalf[s, q * 64] and start[s, k] == start[s, q * 64]
            assert len(at) == 0 or at.max() < 2 * L.entries
            # grid-compaction order: while every residue class (position mod 32) still has a
            # position, entry e comes from class (k + e) mod 32 -- 32 genes, 32 distinct bank slots
            cls = np.bincount(want % 32, minlength=32)
            full = int(cls.min()) * 32
            assert np.array_equal(vals[:full] % 32, (k + np.arange(full)) % 32)
    # (3) r
    dense = eng.associate(gm, trv, mkv, permutations=P, seed=9, use_lists=False)
    res = eng.associate(gm, trv, mkv, permutations=P, seed=9, use_lists=True)
    assert np.array_equal(res["r"].cpu().numpy(), dense["r"].cpu().numpy())
    assert np.array_equal(res["r"].cpu().numpy().view(np.uint32),
                          orc.permute_r(orc.pack_rows(genes), tb, mb, N, P, 9).T)


# ------------------------------------------------ spec S4 at the widths where a block keeps fewer bits ------
@pytest.mark.parametrize("N,T,P,base", [(39_684, 1, 40, 0), (39_685, 2, 33, 64), (77_041, 1, 70, 31),
                                        (145_521, 1, 20, 5), (300_000, 2, 9, 0), (654_848, 1, 3, 1)])
def test_perm_labels_bit_exact_beyond_one_dword_per_row(eng, orc, N, T, P, base):
    """The label generator keeps a block's rows in LDS: all 32 permutations of a Philox block per row
    up to N = 39 684, then 16, 8, 4, 2 and finally 1 of them (N <= 654 848 = scoary_perm_max_isolates;
    the list-driven kernels stop at 131 070, the dense ones and the tree stage take the row form at
    any width).  Every width class against the oracle, with a base that is no multiple of 32."""
    rng = np.random.default_rng(N % 1000 + T)
    traits = (rng.random((T, N)) < 0.3).astype(np.uint8)
    traits[T - 1, rng.random(N) < 0.05] = 2
    tb, mb = _bits(eng, traits)
    masks = eng.vecrows(mb, N)
    margins = __import__("torch").tensor([[int((traits[t] == 1).sum()), int((traits[t] != 2).sum())] for t in range(T)],
                                         dtype=__import__("torch").int32, device="cuda")
    perms = eng.perm_generate(masks, margins, N, P, base, 99).cpu().numpy().view(np.uint32)
    W = (N + 63) // 64
    for t in range(T):
        npos = int((traits[t] == 1).sum())
        for j in sorted({0, 1, P // 2, P - 1}):
            want = orc.perm_labels(99, t, base + j, mb[t], npos, N)
            got = np.ascontiguousarray(perms[t, j, :2 * W]).view(np.uint64)
            assert np.array_equal(got, want), (t, j)
            assert not perms[t, j, 2 * W:].any()


def test_perm_labels_per_lane_mark_counters_do_not_wrap(eng, orc):
    """a lane counts its round-0 marks in 10 bit-sliced planes (<= 1023).  With
    >= 512 blocks in the launch the generator kept 256 threads per block, so at N > 261 888 a thread
    owned up to 2 558 rows and a ~50 % trait (q near 128) wrapped the count: K came out 1024 short per
    overflowed lane, the fix-up ADDED the difference, and the permuted labels no longer had npos
    positives.  The launch now widens the block until a thread has at most 1023 rows.  N = 654 848
    (the largest the generator takes) and N = 300 000, a 50 % trait, P = 1024 (a launch of >= 512
    blocks): every permutation has exactly npos positives among the valid isolates, and selected
    permutations equal the oracle bit for bit."""
    import torch
    for N, P in ((654_848, 1024), (300_000, 1056)):
        rng = np.random.default_rng(N % 977)
        traits = (rng.random((1, N)) < 0.5).astype(np.uint8)
        traits[0, rng.random(N) < 0.01] = 2
        tb, mb = _bits(eng, traits)
        npos, nval = int((traits[0] == 1).sum()), int((traits[0] != 2).sum())
        masks = eng.vecrows(mb, N)
        margins = torch.tensor([[npos, nval]], dtype=torch.int32, device="cuda")
        perms = eng.perm_generate(masks, margins, N, P, 0, 31337)
        W = (N + 63) // 64
        # positives per permutation, counted on the host from the bit rows (32-bit words)
        host = perms.cpu().numpy().view(np.uint32)[0]                       # [P, Wp]
        ones = np.bitwise_count(host[:, :2 * W]).sum(axis=1, dtype=np.int64)
        assert np.array_equal(ones, np.full(P, npos)), (N, int(ones.min()), int(ones.max()), npos)
        mask32 = np.ascontiguousarray(mb[0]).view(np.uint32)
        assert not (host[:, :2 * W] & ~mask32[None, :]).any()               # labels only on valid isolates
        for j in (0, 517, P - 1):
            want = orc.perm_labels(31337, 0, j, mb[0], npos, N)
            assert np.array_equal(np.ascontiguousarray(host[j, :2 * W]).view(np.uint64), want), (N, j)
        del perms, host


def test_perm_labels_every_margin_of_small_traits(eng, orc):
    """Spec S4 at its corners: every (valid isolates, positives) pair of traits over N = 1 ... 9 and a
    few over N = 33 / 70 -- no positives, all positive, one valid isolate, the complemented side,
    round-0 probability zero -- rows and tiles against the oracle, all in one launch per N."""
    import torch
    for N in (1, 2, 3, 5, 9, 33, 70):
        cases = []
        for nval in sorted({1, 2, 3, N // 2, N - 1, N} - {0}):
            if nval > N:
                continue
            for npos in sorted({0, 1, nval // 2, nval - 1, nval} - {-1}):
                if 0 <= npos <= nval:
                    cases.append((nval, npos))
        cases = sorted(set(cases))
        T, P = len(cases), 96
        rng = np.random.default_rng(N)
        traits = np.full((T, N), 2, dtype=np.uint8)
        for t, (nval, npos) in enumerate(cases):
            idx = rng.permutation(N)[:nval]
            traits[t, idx] = 0
            traits[t, idx[:npos]] = 1
        tb, mb = _bits(eng, traits)
        masks = eng.vecrows(mb, N)
        margins = torch.tensor([[npos, nval] for nval, npos in cases], dtype=torch.int32, device="cuda")
        rows = eng.perm_generate(masks, margins, N, P, 0, 2024).cpu().numpy().view(np.uint32)
        tiles = eng.perm_generate_tiles(masks, margins, N, P, 0, 2024).cpu().numpy().view(np.uint32)
        tw, stride, _g, _c, _p = eng.list_params(N)
        tile_words = int(eng.lib.scoary_list_tile_words(N))
        tiles = tiles.reshape(T, -1, tile_words)[:, :, :(N + 1) * tw].reshape(T, -1, N + 1, tw)
        W = (N + 63) // 64
        for t, (nval, npos) in enumerate(cases):
            want = np.stack([orc.perm_labels(2024, t, pi, mb[t], npos, N) for pi in range(P)])
            got = np.ascontiguousarray(rows[t, :, :2 * W]).view(np.uint64).reshape(P, W)
            assert np.array_equal(got, want), (N, nval, npos)
            wbits = np.unpackbits(want.view(np.uint8), axis=1, bitorder="little")[:, :N]        # (P, N)
            tbits = np.unpackbits(np.ascontiguousarray(tiles[t, 0, :N]).view(np.uint8), axis=1,
                                  bitorder="little")[:, :P]                                       # (N, P)
            assert np.array_equal(tbits.T, wbits), (N, nval, npos)
            assert np.all(wbits.sum(axis=1) == npos)


@pytest.mark.parametrize("use_lists", [True, False], ids=["lists", "dense"])
def test_empirical_p_estimates_the_fisher_p_it_is_the_permutation_null_of(eng, use_lists):
    """A check of the LAW, independent of the oracle and of spec S4 (VERDICT r5, weak #1a: oracle and kernel
    share S4, so a defect of the law would pass bit-exact parity).  Under a uniformly random relabelling with the
    margins fixed, the table count a is hypergeometric -- so P(w(a_pi) <= w(a_obs) gamma) IS the two-sided
    Fisher p, and r is a Binomial(P, p) draw around the p-value k_fisher computed (itself pinned to SciPy).
    Every (trait, gene) with 0.02 < p < 0.98 gives a z-score; a sampler that favoured some isolates (by
    position, by word, by validity) would shift the z of the genes that live there -- hence the structured
    genes: index blocks, stripes, word-aligned runs, the isolates next to the missing ones."""
    import torch
    rng = np.random.default_rng(20261002)
    G, N, T, P = 3000, 1999, 4, 20000
    genes = (rng.random((G, N)) < rng.uniform(0.03, 0.97, (G, 1))).astype(np.uint8)
    idx = np.arange(N)
    structured = [idx < N // 2, idx < N // 4, idx >= N - 150, idx % 2 == 0, idx % 64 < 32, idx % 64 == 63,
                  (idx // 64) % 2 == 0, idx % 7 == 0, idx < 64, (idx > 700) & (idx < 1300), idx % 32 == 0,
                  rng.random(N) < idx / N, rng.random(N) < (1 - idx / N) ** 2]
    for k, pat in enumerate(structured):
        for j in range(8):                                       # the pattern and noisy copies of it
            genes[10 + 8 * k + j] = pat ^ (rng.random(N) < 0.02 * j)
    traits = (rng.random((T, N)) < np.array([[0.5], [0.12], [0.8], [0.35]])).astype(np.uint8)
    traits[1, rng.random(N) < 0.07] = 2                          # missing values in two traits
    traits[3, (idx % 64 == 5) | (idx > N - 40)] = 2
    tb, mb = _bits(eng, traits)
    gm = eng.pack_dense(genes)
    trv, mkv = eng.vecrows(tb, N), eng.vecrows(mb, N)
    if use_lists:
        eng.build_lists(gm)
    zs = []
    for seed in (11, 12):                                        # two independent sets of permutations
        res = eng.associate(gm, trv, mkv, permutations=P, seed=seed, use_lists=use_lists)
        torch.cuda.synchronize()
        p = res["p"].cpu().numpy()
        r = res["r"].cpu().numpy().view(np.uint32).astype(np.float64)
        c = res["counts"].cpu().numpy()
        tested = ((c[..., 0] + c[..., 2]) > 0) & ((c[..., 1] + c[..., 3]) > 0) & (p > 0.02) & (p < 0.98)
        z = (r - P * p) / np.sqrt(P * p * (1 - p))
        assert tested.sum() > 8000
        zs.append(np.where(tested, z, np.nan))
        zt = z[tested]
        assert np.max(np.abs(zt)) < 5.5, float(np.max(np.abs(zt)))
        assert 0.85 < np.mean(zt ** 2) < 1.15, float(np.mean(zt ** 2))
        assert abs(np.mean(zt)) < 0.08, float(np.mean(zt))
        assert 0.03 < np.mean(np.abs(zt) > 2) < 0.065
        zs_struct = z[:, 10:10 + 8 * len(structured)][tested[:, 10:10 + 8 * len(structured)]]
        # (13 patterns x 8 near-copies: the mean has the spread of ~13 values, 0.28; a block of isolates the
        # sampler under- or over-uses by 1 % moves the z of its genes by several units at P = 20 000)
        assert len(zs_struct) > 100 and np.max(np.abs(zs_struct)) < 4.8 and abs(np.mean(zs_struct)) < 0.9
    # the two seeds are independent draws: their z-scores are uncorrelated gene by gene
    both = ~np.isnan(zs[0]) & ~np.isnan(zs[1])
    assert abs(np.corrcoef(zs[0][both], zs[1][both])[0, 1]) < 0.05
