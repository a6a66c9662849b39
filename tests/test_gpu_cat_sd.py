"""The step-down kernels of the categorical traits (spec S23) on the GPU against the plain-numpy restatement
(cat_sd_spec.py on top of cat_wy_spec.py, categorical_spec.py and gcmh_spec.py): the order, the raw counts by rank, r_sd
and the maxima bit for bit, through the raw entry points and through the engine -- at the run and supergroup boundaries
(G = 1 .. 2049), at one isolate, word tails, one and two chunks of isolates, stage tails, three and seven class planes,
empty classes, a trait of one class, isolates without a label, a class confined to one stratum, garbage behind the
rows, sentinels behind the counters and behind every row of maxs, counters that start at 5 -- and on planted inputs:
tie groups across the run and supergroup boundaries, a trait whose genes all tie, a maximum in the last run only and at
rank 0 only, blocks that walk several supergroups, an order entry that is no gene, batches, refusals."""
import numpy as np
import pytest

import cat_sd_spec as sd
import cat_wy_spec as ws
import categorical_spec as cs
import gcmh_spec as gs

pytestmark = pytest.mark.gpu
SEED = 0x5EED23C4
ERR_ARG, ERR_SIZE = -1, -3
CHUNK = 2432                                   # isolates of a chunk of the kernels (kCatChunk)
SENTINEL = -7.25                               # behind every row of maxs: no maximum of s is negative
ISENTINEL = -123456                            # behind the counters
# name: (N, G, P, strata of the gcmh run)
SHAPES = {"g1": (1, 1, 1, 1), "g3": (31, 3, 63, 5), "g4": (33, 4, 64, 1), "g5": (CHUNK, 5, 65, 4),
          "g63": (CHUNK + 1, 63, 130, 2), "g64": (31, 64, 65, 5), "g65": (33, 65, 130, 2), "g1023": (31, 1023, 63, 5),
          "g1024": (33, 1024, 64, 1), "g1025": (CHUNK + 1, 1025, 65, 2), "g2049": (33, 2049, 130, 3)}
CASES = tuple(SHAPES)
TESTS = ("chi2", "gcmh")


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _shape(name):
    """(genes [G, N] 0/1, codes [T, N], strata [N]): T = 5 traits of different K -- three classes with missing
    isolates (three planes), eight classes (seven planes), an empty class in the middle, one class only (every gene
    untestable) and five classes of which the last lives in one stratum alone (a rank-deficient form)."""
    N, G, _P, S = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if N == 31:
        strata = np.repeat(np.arange(5), [12, 12, 4, 2, 1])              # strata of 2 and 1 isolates
    else:
        strata = rng.integers(0, S, N)
        strata[N - 1] = S - 1
    k3 = rng.integers(0, 4, N)
    k8 = rng.integers(1, 9, N)
    gap = rng.choice([0, 1, 3], N)
    one = (rng.random(N) < 0.8).astype(np.int64)
    only5 = rng.integers(1, 5, N)
    only5[(strata == 0) & (rng.random(N) < 0.4)] = 5                    # class 5 is confined to stratum 0
    codes = np.stack([k3, k8, gap, one, only5]).astype(np.int64)
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    if G > 8:
        genes[1] = 0                           # m = 0
        genes[2] = 1                           # m = n
        genes[3] = codes[0] == 0               # carried only by isolates without a label (first trait)
        genes[4] = codes[1] == 1               # equal to a class of the second trait: X2 = n, the largest there is
        genes[5, strata == 0] = 0              # absent from the stratum that holds class 5
        genes[7] = genes[6]                    # a tie group of two
    return genes, codes, strata


def _garbage_behind(eng, rows):
    """The rows [T, P, N] at the front of a buffer whose rest -- where a stage's pad permutations would be read --
    holds codes of every class."""
    import torch
    T, P, N = rows.shape
    buf = torch.randint(1, 9, ((T * P + 64) * N,), dtype=torch.int16, device=eng.device)
    buf[:T * P * N] = rows.reshape(-1)
    return buf[:T * P * N].view(T, P, N)


def _counter(eng, T, G, start):
    """int32 [T, G] of ``start`` at the front of a buffer with sentinels behind it: (the view, the whole buffer)."""
    import torch
    buf = torch.full((T * G + 5,), ISENTINEL, dtype=torch.int32, device=eng.device)
    buf[:T * G] = start
    return buf[:T * G].view(T, G), buf


def _maxs_with_sentinels(eng, T, P, fill=0.0):
    import torch
    maxs = torch.full((T, P + 3), fill, dtype=torch.float64, device=eng.device)
    maxs[:, P:] = SENTINEL
    return maxs


class Side:
    """One test's observed side on the device: what the gather and a batch take."""
    def __init__(self, eng, test, genes, codes, strata, seed=SEED):
        self.eng, self.test, self.gm, self.seed = eng, test, eng.pack_dense(genes), seed
        if test == "chi2":
            self.plan = eng.categorical_plan(codes)
            self.obs = eng.categorical(self.gm, self.plan)
            self.inv, self.ivm, _sobs, self.thr = eng.categorical_wy_prepare(self.plan, self.obs["a"])
        else:
            self.plan = eng.gcmh_plan(codes, strata)
            self.obs = eng.gcmh(self.gm, self.plan)
            self.form, self.thr = self.obs["form"], self.obs["thr"]

    def rows(self, base, P):
        return (self.eng.categorical_rows if self.test == "chi2" else self.eng.gcmh_rows)(self.plan, base, P, self.seed)

    def gather(self, order32, batch, thr=None, ivm=None, form=None):
        thr = self.thr if thr is None else thr
        if self.test == "chi2":
            return self.eng.cat_stepdown_gather(self.gm, order32, self.obs["a"], self.ivm if ivm is None else ivm, thr,
                                                self.plan.N, batch)
        return self.eng.gcmh_stepdown_gather(self.gm, order32, self.form if form is None else form, thr, self.plan.N,
                                             batch)

    def batch(self, scratch, rows, base, r_rank, c_rank, maxs):
        if self.test == "chi2":
            self.eng.permute_cat_stepdown(scratch, self.plan, self.inv, rows, self.gm.G, base, r_rank, c_rank, maxs)
        else:
            self.eng.permute_gcmh_stepdown(scratch, self.plan, rows, self.gm.G, base, r_rank, c_rank, maxs)

    def plain(self, rows, r):
        if self.test == "chi2":
            return self.eng.permute_categorical(self.gm, self.plan, self.obs["a"], rows, r)
        return self.eng.permute_gcmh(self.gm, self.plan, self.obs, rows, r)

    def stepdown(self, P, budget=8 << 30):
        f = self.eng.categorical_stepdown if self.test == "chi2" else self.eng.gcmh_stepdown
        return f(self.gm, self.plan, self.obs, P, self.seed, budget_bytes=budget)

    def westfall_young(self, P):
        f = self.eng.categorical_westfall_young if self.test == "chi2" else self.eng.gcmh_westfall_young
        return f(self.gm, self.plan, self.obs, P, self.seed)


def _trait(test, genes, codes_t, strata, S, rows_t):
    if test == "chi2":
        return sd.chi2_trait(genes, codes_t, rows_t)
    return sd.gcmh_trait(genes, codes_t, strata, S, rows_t)


def _two_batch_budget(T, N, G):
    return 2 * 64 * T * N + 8 * T * (-(-G // 1024) * 16) * 64              # cat_stepdown_batch() = 64 under it


_CACHE = {}


def _run(eng, test, name):
    """A shape's run of one test, computed once: the raw entry points on the rows read back (counters from 5, sentinels
    everywhere), the engine from the seed (two batches where P allows it), S22's engine route, and the restatement."""
    if (test, name) in _CACHE:
        return _CACHE[(test, name)]
    genes, codes, strata = _shape(name)
    N, G, P, S = SHAPES[name]
    T = codes.shape[0]
    side = Side(eng, test, genes, codes, strata)
    rows = side.rows(0, P)
    padded = _garbage_behind(eng, rows)
    order32, tt = eng.rank_stepdown_order(side.thr)
    scratch = side.gather(order32, P)
    (r_rank, r_buf), (c_rank, c_buf), (p5, _pb) = (_counter(eng, T, G, 5) for _ in range(3))
    maxs = _maxs_with_sentinels(eng, T, P, fill=3.5)                     # (a write, not a combine: 3.5 must go)
    side.batch(scratch, padded, 0, r_rank, c_rank, maxs)
    side.plain(padded, p5)
    r, r_fwer, r_sd, emaxs = side.stepdown(P, budget=(8 << 30) if P <= 128 else _two_batch_budget(T, N, G))
    wy = side.westfall_young(P)
    rows_h = rows.cpu().numpy()
    spec = []
    for t in range(T):
        tr = _trait(test, genes, codes[t], strata, S, rows_h[t])
        tr["sd"] = sd.stepdown(tr["cells"], tr["thr"])
        tr["maxs"] = ws.maxs(tr["cells"])
        spec.append(tr)
    dev = {k: v.cpu().numpy() for k, v in dict(order=order32, tt=tt, r_rank=r_rank, c_rank=c_rank, r_buf=r_buf,
                                                c_buf=c_buf, p5=p5, maxs=maxs, r=r, r_fwer=r_fwer, r_sd=r_sd,
                                                emaxs=emaxs, wy_r=wy[0], wy_fwer=wy[1], wy_maxs=wy[2]).items()}
    _CACHE[(test, name)] = dict(spec=spec, dev=dev)
    return _CACHE[(test, name)]


def test_the_shapes_reach_every_boundary():
    assert sorted(s[1] for s in SHAPES.values()) == [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049]
    assert {s[0] for s in SHAPES.values()} == {1, 31, 33, CHUNK, CHUNK + 1}
    assert {s[2] for s in SHAPES.values()} == {1, 63, 64, 65, 130}
    _genes, codes, strata = _shape("g3")
    assert sorted(np.bincount(strata))[:2] == [1, 2] and 1 in {s[3] for s in SHAPES.values()}
    assert [int(row.max()) for row in codes] == [3, 8, 3, 1, 5] and 2 not in codes[2] and 0 in codes[0]
    assert set(strata[codes[4] == 5]) == {0}
    assert _two_batch_budget(5, 33, 2049) // (2 * 64 * 5 * 33 + 8 * 5 * 48 * 64) * 64 == 64


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("test", TESTS)
def test_order_counts_and_maxima_are_the_restatement_bit_for_bit(eng, test, name):
    c = _run(eng, test, name)
    N, G, P, _S = SHAPES[name]
    dev = c["dev"]
    assert (dev["maxs"][:, P:] == SENTINEL).all()                        # nothing behind a row's P columns
    assert (dev["r_buf"][-5:] == ISENTINEL).all() and (dev["c_buf"][-5:] == ISENTINEL).all()
    for t, tr in enumerate(c["spec"]):
        out = tr["sd"]
        assert np.array_equal(dev["order"][t], out["order"]), (name, t)
        assert np.array_equal(_bits(dev["tt"][t]), _bits(out["tt"])), (name, t)
        assert np.array_equal(dev["c_rank"][t] - 5, out["c"]), (name, t)
        # pass A's count, scattered, is the plain kernel's on the same rows, from 5 -- and the restatement's
        assert np.array_equal(dev["r_rank"][t], dev["p5"][t][out["order"]]), (name, t)
        assert np.array_equal(dev["r_rank"][t] - 5, tr["r"][out["order"]]), (name, t)
        # u[0], written over what the cell held
        assert np.array_equal(_bits(dev["maxs"][t, :P]), _bits(tr["maxs"])), (name, t)
        assert np.array_equal(_bits(out["u"][0]), _bits(tr["maxs"]))
        # the engine, from the seed
        assert np.array_equal(dev["r_sd"][t], out["r_sd"]), (name, t)
        assert np.array_equal(dev["r"][t], tr["r"]), (name, t)
        assert np.array_equal(_bits(dev["emaxs"][t]), _bits(tr["maxs"])), (name, t)
        assert np.array_equal(dev["r_fwer"][t], ws.r_fwer(tr["maxs"], tr["thr"])), (name, t)
        assert (dev["r"][t] <= dev["r_sd"][t]).all() and (dev["r_sd"][t] <= dev["r_fwer"][t]).all(), (name, t)
        top = tr["thr"] == tr["thr"].max()
        assert np.array_equal(dev["r_sd"][t][top], dev["r_fwer"][t][top])
        assert (dev["r_sd"][t][tr["thr"] == 0] == P).all()
        if G == 1:
            assert np.array_equal(dev["r_sd"][t], dev["r_fwer"][t])
    # r, r_fwer and maxs are S22's route, bit for bit
    assert np.array_equal(dev["r"], dev["wy_r"]) and np.array_equal(dev["r_fwer"], dev["wy_fwer"])
    assert np.array_equal(_bits(dev["emaxs"]), _bits(dev["wy_maxs"]))
    one = 3                                                              # the trait of one class: maxs = 0, r_sd = P
    assert not dev["maxs"][one, :P].any() and (dev["r_sd"][one] == P).all() and (dev["c_rank"][one] - 5 == P).all()
    if N > 1:
        assert (dev["maxs"][1, :P] > 0).all()


def _planted(eng, test):
    """G = 1100 -- a full supergroup and a ragged one, whose last run holds the ranks 1088 .. 1099 -- with the values
    the passes compare against planted through the raw entry points: the kernels take thr, ivm and the forms as they
    are handed in, and so does the restatement.  Trait 0: tie groups across the ranks 0/1, 3/4, 63/64 and 1023/1024;
    trait 1: every gene ties; trait 2: a statistic above 0 in the last run only; trait 3: at rank 0 only."""
    import torch
    if ("planted", test) in _CACHE:
        return _CACHE[("planted", test)]
    rng = np.random.default_rng(1100)
    N, G, P, S, T = 33, 1100, 65, 3, 4
    genes = (rng.random((G, N)) < rng.uniform(0.1, 0.9, (G, 1))).astype(np.uint8)
    row3, row8 = rng.integers(0, 4, N), rng.integers(1, 9, N)
    codes = np.stack([row3, row8, row3, row8])
    strata = rng.integers(0, S, N)
    strata[0] = S - 1
    side = Side(eng, test, genes, codes, strata)
    thr = side.thr.cpu().numpy().copy()
    live = np.ones((T, G), dtype=bool)
    thr[2] = thr[2][rng.permutation(G)]            # (any gene may stand in the last run, not the untestable ones)
    order = [sd.order_of(thr[t]) for t in range(T)]
    for lo in (0, 3, 63, 1023):
        thr[0, order[0][lo + 1]] = thr[0, order[0][lo]]
    thr[1, :] = np.median(thr[1])
    live[2, order[2][:1088]] = False
    live[3, order[3][1:]] = False
    dthr = torch.from_numpy(thr).to(eng.device)
    dlive = torch.from_numpy(live).to(eng.device)
    kw = dict(thr=dthr)
    if test == "chi2":
        kw["ivm"] = (side.ivm * dlive).contiguous()
    else:
        kw["form"] = (side.form * dlive[:, :, None]).contiguous()
    order32, tt = eng.rank_stepdown_order(dthr)
    rows = side.rows(0, P)
    (r_rank, _), (c_rank, _) = _counter(eng, T, G, 0), _counter(eng, T, G, 0)
    maxs = _maxs_with_sentinels(eng, T, P)
    side.batch(side.gather(order32, P, **kw), rows, 0, r_rank, c_rank, maxs)
    rows_h = rows.cpu().numpy()
    spec = []
    for t in range(T):
        tr = _trait(test, genes, codes[t], strata, S, rows_h[t])
        cells = tr["cells"] * live[t][None]                                  # ivm 0 / a form of zeros: s = +0.0
        # pass A's count: S20's integer comparison, or Q >= the thr that was handed in
        r = tr["r"] if test == "chi2" else (cells >= thr[t][None]).sum(axis=0)
        spec.append(dict(r=r, cells=cells, sd=sd.stepdown(cells, thr[t])))
    _CACHE[("planted", test)] = dict(side=side, order32=order32, kw=kw, rows=rows, thr=thr, spec=spec,
                dev={k: v.cpu().numpy() for k, v in dict(order=order32, tt=tt, r_rank=r_rank, c_rank=c_rank,
                                                         maxs=maxs).items()})
    return _CACHE[("planted", test)]


@pytest.mark.parametrize("test", TESTS)
def test_planted_ties_and_maxima(eng, test):
    import torch
    c = _planted(eng, test)
    dev, P, G = c["dev"], 65, 1100
    for t, sp in enumerate(c["spec"]):
        out = sp["sd"]
        assert np.array_equal(dev["order"][t], out["order"]), t
        assert np.array_equal(dev["c_rank"][t], out["c"]), t
        assert np.array_equal(_bits(dev["maxs"][t, :P]), _bits(out["u"][0])), t
        assert np.array_equal(dev["r_rank"][t], sp["r"][out["order"]]), t
    tt = dev["tt"]
    for lo in (0, 3, 63, 1023):
        assert tt[0, lo] == tt[0, lo + 1]
    assert len(set(tt[1].tolist())) == 1
    r_sd = eng.rank_stepdown_tail(torch.from_numpy(dev["c_rank"].astype(np.int32)).to(eng.device),
                                  torch.from_numpy(tt).to(eng.device), c["order32"]).cpu().numpy()
    for t, sp in enumerate(c["spec"]):
        assert np.array_equal(r_sd[t], sp["sd"]["r_sd"]), t
    # the trait whose genes all tie: one count for all of them, the single-step one
    assert len(set(r_sd[1].tolist())) == 1 and r_sd[1, 0] == (dev["maxs"][1, :P] >= c["thr"][1, 0]).sum()
    # the maximum in the last run only: every run in front of it takes it over through the suffix
    u = c["spec"][2]["sd"]["u"]
    assert (u[0] > 0).any() and np.array_equal(_bits(u[0]), _bits(u[1088]))
    assert not c["spec"][2]["cells"][:, c["spec"][2]["sd"]["order"][:1088]].any()
    # the maximum at rank 0 only: behind it u is 0 and only thr = 0 is reached
    u = c["spec"][3]["sd"]["u"]
    assert (u[0] > 0).any() and not u[1:].any()
    assert np.array_equal(dev["c_rank"][3][1:], np.where(dev["tt"][3][1:] == 0, P, 0))


@pytest.mark.parametrize("test", TESTS)
def test_an_order_entry_that_is_no_gene_makes_a_pad_position(eng, test):
    c = _planted(eng, test)
    side, G, P, T = c["side"], 1100, 65, 4
    order2 = c["order32"].clone()
    order2[0, 5] = G + 7
    order2[1, G - 1] = -1
    order2[2, 1090] = 1 << 30
    (r_rank, _), (c_rank, _) = _counter(eng, T, G, 0), _counter(eng, T, G, 0)
    maxs = _maxs_with_sentinels(eng, T, P)
    side.batch(side.gather(order2, P, **c["kw"]), c["rows"], 0, r_rank, c_rank, maxs)
    c_rank, maxs, r_rank = c_rank.cpu().numpy(), maxs.cpu().numpy(), r_rank.cpu().numpy()
    for t, k in ((0, 5), (1, G - 1), (2, 1090), (3, None)):
        sp = c["spec"][t]
        order = sp["sd"]["order"].copy()
        cells = np.concatenate([sp["cells"], np.zeros((P, 1))], axis=1)      # column G: the pad position's s = 0
        tt = c["thr"][t][order]
        if k is not None:
            order[k], tt[k] = G, np.inf
        u = sd.successive_maxima(cells, order)
        want = sd.raw_counts(u, tt)
        assert np.array_equal(c_rank[t], want), t
        assert k is None or c_rank[t, k] == 0
        assert np.array_equal(_bits(maxs[t, :P]), _bits(u[0])), t
        keep = np.arange(G) != (-1 if k is None else k)
        assert np.array_equal(r_rank[t][keep], sp["r"][sp["sd"]["order"]][keep]), t


def test_blocks_that_walk_several_supergroups(eng):
    """More supergroups than a launch has ranges (32 traits of one stage: at most 32 ranges on 256 CUs): a block's
    loop over supergroups, its pointer into gmax and its reset of the run maximum, at N = 33."""
    rng = np.random.default_rng(33)
    N, G, P, T, S = 33, 1024 * 40 + 3, 3, 32, 3
    genes = (rng.random((G, N)) < rng.uniform(0.0, 1.0, (G, 1))).astype(np.uint8)
    codes = np.stack([rng.integers(0, 4, N) if t % 2 else rng.integers(1, 9, N) for t in range(T)])
    strata = rng.integers(0, S, N)
    strata[0] = S - 1
    for test in TESTS:
        side = Side(eng, test, genes, codes, strata)
        r, r_fwer, r_sd, maxs = (x.cpu().numpy() for x in side.stepdown(P))
        wy = [x.cpu().numpy() for x in side.westfall_young(P)]
        assert np.array_equal(r, wy[0]) and np.array_equal(r_fwer, wy[1]) and np.array_equal(_bits(maxs), _bits(wy[2]))
        rows = side.rows(0, P).cpu().numpy()
        thr = side.thr.cpu().numpy()
        for t in range(0, T, 7):
            a_perm = sd.tables(genes, rows[t])                               # [P, G, 8]
            if test == "chi2":                                               # (ivm and the forms: checked elsewhere)
                nk = cs.sizes(codes[t].tolist(), 8)
                ivm = side.ivm[t].cpu().numpy()
                assert ivm[0] == ws.ivm_of(sd.tables(genes[:1], codes[t])[0].tolist(), nk)
                cells = ws.stats(a_perm, nk, ivm)
            else:
                cells = gs.q_many(a_perm, side.form[t].cpu().numpy())
            out = sd.stepdown(cells, thr[t])
            assert np.array_equal(r_sd[t], out["r_sd"]), (test, t)
            assert np.array_equal(_bits(maxs[t]), _bits(out["u"][0])), (test, t)


@pytest.mark.parametrize("test", TESTS)
def test_two_batches_of_64_against_one_of_128_and_a_repeat(eng, test):
    genes, codes, strata = _shape("g65")
    T, N, G, P = codes.shape[0], codes.shape[1], len(genes), 128
    side = Side(eng, test, genes, codes, strata)
    one = side.stepdown(P)
    assert eng.cat_stepdown_batch(G, T, N, P, _two_batch_budget(T, N, G)) == 64
    assert eng.cat_stepdown_batch(G, T, N, P) == 128
    two = side.stepdown(P, budget=_two_batch_budget(T, N, G))
    again = side.stepdown(P)
    for x, y, z in zip(one, two, again):                                 # (r, r_fwer, r_sd, maxs)
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(z.cpu().numpy()))
    # the raw route: perm_base places a batch's maxima, and the counters add
    order32, _tt = eng.rank_stepdown_order(side.thr)
    scratch = side.gather(order32, 64)
    (r_rank, _), (c_rank, _) = _counter(eng, T, G, 0), _counter(eng, T, G, 0)
    maxs = _maxs_with_sentinels(eng, T, P)
    for base in (64, 0):                                                 # (in either order)
        side.batch(scratch, side.rows(base, 64), base, r_rank, c_rank, maxs)
    assert np.array_equal(_bits(maxs[:, :P].cpu().numpy()), _bits(one[3].cpu().numpy()))
    assert (maxs[:, P:].cpu().numpy() == SENTINEL).all()
    r = np.empty((T, G), dtype=np.int32)
    np.put_along_axis(r, order32.cpu().numpy().astype(np.int64), r_rank.cpu().numpy(), axis=1)
    assert np.array_equal(r, one[0].cpu().numpy())
    assert np.array_equal(eng.rank_stepdown_tail(c_rank, _tt, order32).cpu().numpy(), one[2].cpu().numpy())


@pytest.mark.parametrize("test", TESTS)
def test_the_planted_driver_through_the_engine(eng, test):
    genes, codes, strata, tr, out, r_fwer = sd.planted_problem(test)
    side = Side(eng, test, genes, codes[None, :], strata, seed=sd.PLANTED_SEED)
    r, e_fwer, r_sd, maxs = (x.cpu().numpy()[0] for x in side.stepdown(sd.PLANTED_P))
    assert np.array_equal(r, tr["r"]) and np.array_equal(e_fwer, r_fwer) and np.array_equal(r_sd, out["r_sd"])
    assert np.array_equal(_bits(maxs), _bits(out["u"][0]))
    assert (r_sd < e_fwer).any() and (r <= r_sd).all() and (r_sd <= e_fwer).all()


def test_sizes_past_the_limits_and_bad_bases_are_refused_with_nothing_written(eng):
    import torch
    G, T, N, P, S = 10, 1, 40, 5, 2
    gm = eng.pack_dense(np.ones((G, N), dtype=np.uint8))
    codes = (np.arange(N) % 3 + 1).reshape(1, N)
    plan = eng.categorical_plan(codes)
    gplan = eng.gcmh_plan(codes, np.arange(N) % S)
    obs, gobs = eng.categorical(gm, plan), eng.gcmh(gm, gplan)
    inv, ivm, _sobs, thr = eng.categorical_wy_prepare(plan, obs["a"])
    order32, _tt = eng.rank_stepdown_order(thr)
    pat = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=eng.device)        # noqa: E731
    r, c, maxs = pat((T, G), torch.int32), pat((T, G), torch.int32), pat((T, P + 3), torch.float64)
    rows = torch.zeros((T, P, N), dtype=torch.int16, device=eng.device)
    ptr, lib = eng._ptr, eng.lib
    big = eng.ranksum_max_isolates() + 1
    need = [int(lib.scoary_cat_stepdown_scratch_bytes(eng.h, G, T, N, P, k)) for k in (0, 1)]
    Gs, Qs = 1024, 1
    assert need[0] == T * (Qs * Gs * 16 + Gs * (32 + 8 + 8) + (Gs // 64) * 64 * 8)
    assert need[1] == T * (Qs * Gs * 16 + Gs * (35 * 8 + 8) + (Gs // 64) * 64 * 8)
    assert need[0] - int(lib.scoary_cat_stepdown_scratch_bytes(eng.h, G, T, N, 65, 0)) == -T * (Gs // 64) * 64 * 8
    for g, t, n, pp in ((0, T, N, P), (G, 0, N, P), (G, T, 0, P), (G, T, N, 0), ((1 << 31) - 1024, T, N, P)):
        assert lib.scoary_cat_stepdown_scratch_bytes(eng.h, g, t, n, pp, 0) == 0
    assert lib.scoary_cat_stepdown_scratch_bytes(None, G, T, N, P, 0) == 0
    scratch = pat((max(need),), torch.uint8)

    def chi2(g, t, n, pp, base, stride):
        return lib.scoary_permute_cat_stepdown(eng.h, ptr(scratch), ptr(rows), ptr(plan.nk), ptr(plan.w), ptr(inv), g,
                                               t, n, pp, base, ptr(r), ptr(c), ptr(maxs), stride, eng._stream())

    def gcmh(g, t, n, pp, base, stride):
        return lib.scoary_permute_gcmh_stepdown(eng.h, ptr(scratch), ptr(rows), ptr(gplan.nk), g, t, n, pp, base,
                                                ptr(r), ptr(c), ptr(maxs), stride, eng._stream())

    def gather(g, t, n):
        return lib.scoary_cat_stepdown_gather(eng.h, ptr(gm.tiled), ptr(order32), ptr(obs["a"]), ptr(ivm), ptr(thr), g,
                                              t, n, ptr(scratch), eng._stream())

    def ggather(g, t, n):
        return lib.scoary_gcmh_stepdown_gather(eng.h, ptr(gm.tiled), ptr(order32), ptr(gobs["form"]),
                                               ptr(gobs["thr"]), g, t, n, ptr(scratch), eng._stream())
    for call in (chi2, gcmh):
        for g, t, n, pp in ((G, T, big, P), (G, T, N, 1 << 31), (G, 65536, N, P), (1 << 31, T, N, P),
                            ((1 << 31) - 1024, T, N, P)):
            assert call(g, t, n, pp, 0, max(pp, P) + 3) == ERR_SIZE, (call.__name__, g, t, n, pp)
        assert call(G, T, N, P, -1, P + 3) == ERR_ARG                   # perm_base < 0
        assert call(G, T, N, P, 0, P - 1) == ERR_ARG                    # maxs_stride < perm_base + P
        assert call(G, T, N, P, 4, P + 3) == ERR_ARG
        assert call(G, T, N, 0, 0, P) == ERR_ARG
    for call in (gather, ggather):
        for g, t, n in ((G, T, big), (G, 65536, N), (1 << 31, T, N), ((1 << 31) - 1024, T, N)):
            assert call(g, t, n) == ERR_SIZE, (call.__name__, g, t, n)
        assert call(0, T, N) == ERR_ARG
    torch.cuda.synchronize()
    for x in (r, c, maxs, scratch):
        assert bool((x == 77).all())
    # (the arguments were sound otherwise)
    assert gather(G, T, N) == 0 and chi2(G, T, N, P, 3, P + 3) == 0
    assert ggather(G, T, N) == 0 and gcmh(G, T, N, P, 0, P + 3) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="maxs is the whole float64"):
        eng.permute_cat_stepdown(scratch, plan, inv, rows, G, 0, r, c, maxs.to(torch.float32))
    with pytest.raises(ValueError, match="r is int32"):
        eng.permute_gcmh_stepdown(scratch, gplan, rows, G, 0, r, c[:, :G - 1], maxs)


def test_the_lds_opt_in_is_taken_once_per_kernel_on_a_fresh_engine():
    """The four hot kernels on an engine of their own, first at N = 1152 (64 512 B of LDS: no opt-in), then at N = 1153
    (71 680 B: the kernel's first launch that needs the opt-in), then at N = 1153 again (the handle's bit is set)."""
    from scoary_amd.engine import AssociationEngine
    G, T, P, K, S = 70, 1, 65, 5, 3
    fresh = AssociationEngine(0)
    try:
        for N in (1152, 1153, 1153):
            rng = np.random.default_rng(N)
            genes = (rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))).astype(np.uint8)
            codes = rng.integers(0, K + 1, (T, N))
            strata = rng.integers(0, S, N)
            strata[0] = S - 1
            for test in TESTS:
                side = Side(fresh, test, genes, codes, strata)
                r, r_fwer, r_sd, maxs = (x.cpu().numpy() for x in side.stepdown(P))
                tr = _trait(test, genes, codes[0], strata, S, side.rows(0, P).cpu().numpy()[0])
                out = sd.stepdown(tr["cells"], tr["thr"])
                assert np.array_equal(r[0], tr["r"]) and np.array_equal(r_sd[0], out["r_sd"]), (N, test)
                assert np.array_equal(_bits(maxs[0]), _bits(out["u"][0])), (N, test)
    finally:
        fresh.close()
