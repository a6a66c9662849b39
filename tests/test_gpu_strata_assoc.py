"""associate(strata=...) and the other consumers of stratified labels (spec S9): every count is recomputed on the
host from the downloaded stratified label rows, the regions / p values of the association step, and numpy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 20261018


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    e.set_mfma_route("auto")
    yield e
    e.close()


class Case:
    """Genes, traits and strata on the device, the stratified label bits on the host."""

    def __init__(self, eng, G, N, T, S, P, seed=SEED, dense_genes=False):
        from scoary_amd.engine import pack_bits_rows
        rng = np.random.default_rng(G + N + S)
        lo, hi = (0.3, 0.7) if dense_genes else (0.02, 0.98)
        self.genes = (rng.random((G, N)) < rng.uniform(lo, hi, (G, 1))).astype(np.uint8)
        self.genes[1], self.genes[2] = 0, 1
        self.traits = (rng.random((T, N)) < rng.uniform(0.2, 0.8, (T, 1))).astype(np.uint8)
        self.traits[0] = np.where(rng.random(N) < 0.7, self.genes[3], self.traits[0])      # one strong association
        self.traits[T - 1, rng.random(N) < 0.06] = 2
        self.strata = rng.integers(0, S, N)
        self.G, self.N, self.T, self.S, self.P, self.seed = G, N, T, S, P, seed
        self.gm = eng.pack_dense(self.genes)
        self.trv = eng.vecrows(pack_bits_rows((self.traits == 1).astype(np.uint8)), N)
        self.mkv = eng.vecrows(pack_bits_rows((self.traits != 2).astype(np.uint8)), N)
        self.plan = eng.trait_plan(self.trv, self.mkv, N)
        self.sp = eng.strata_plan(self.strata, self.trv, self.mkv, N)
        rows = eng.perm_generate(self.mkv, self.plan.margins, N, P, 0, seed, strata=self.sp).cpu().numpy()
        bits = np.unpackbits(rows.view(np.uint8).reshape(T, P, -1), axis=2, bitorder="little")[:, :, :N]
        self.labels = bits                                                               # [T, P, N]
        self.a = np.einsum("tpn,gn->tpg", bits.astype(np.int64), self.genes.astype(np.int64))    # overlap counts

    def want_r(self, crit):
        """The interval test on a = popcount(gene & label): extreme iff (uint32)(a - base) >= span."""
        c = crit.cpu().numpy().view(np.uint32).astype(np.int64)
        base, span = c[:, None, :, 0], c[:, None, :, 1]
        return (((self.a - base) & 0xffffffff) >= span).sum(1).astype(np.uint32)

    def want_p_perm(self, eng, counts):
        """p of every (trait, permutation, gene): the association step's own Fisher kernel on the permuted table."""
        import torch
        c = counts.cpu().numpy().astype(np.int64)
        npos, gmar, nval = (c[:, :, 0] + c[:, :, 1])[:, None, :], (c[:, :, 0] + c[:, :, 2])[:, None, :], \
            c.sum(2)[:, None, :]
        tabs = np.stack([self.a, npos - self.a, gmar - self.a, nval - npos - gmar + self.a], axis=3).astype(np.int32)
        p = eng.fisher(torch.from_numpy(tabs.reshape(-1, 4)).to(eng.device), want_crit=False)[0]
        return p.cpu().numpy().reshape(self.T, self.P, self.G)


@pytest.fixture(scope="module")
def case257(eng):
    return Case(eng, 300, 257, 3, 4, 320)


@pytest.mark.parametrize("use_lists", [True, False], ids=["lists", "dense"])
def test_associate_r_equals_the_host_recomputation(eng, case257, use_lists):
    c = case257
    if use_lists and c.gm.lists is None:
        eng.build_lists(c.gm)
    res = eng.associate(c.gm, c.trv, c.mkv, permutations=c.P, seed=c.seed, use_lists=use_lists, strata=c.sp)
    got = res["r"].cpu().numpy().view(np.uint32)
    assert np.array_equal(got, c.want_r(res["crit"]))
    plain = eng.associate(c.gm, c.trv, c.mkv, permutations=c.P, seed=c.seed, use_lists=use_lists)
    assert not np.array_equal(plain["r"].cpu().numpy().view(np.uint32), got)
    for k in ("counts", "p", "crit"):
        assert np.array_equal(plain[k].cpu().numpy(), res[k].cpu().numpy())


def test_associate_r_with_the_matrix_core_kernel(eng):
    c = Case(eng, 512, 600, 2, 5, 512, dense_genes=True)
    eng.set_mfma_route("all")
    try:
        eng.build_lists(c.gm)
        split = eng.mfma_split(c.gm, c.T, c.P)
        if split <= 0:
            pytest.skip("the matrix-core kernel takes no slot of this shape (mfma_split = 0)")
        res = eng.associate(c.gm, c.trv, c.mkv, permutations=c.P, seed=c.seed, use_lists=True, strata=c.sp)
        assert np.array_equal(res["r"].cpu().numpy().view(np.uint32), c.want_r(res["crit"]))
    finally:
        eng.set_mfma_route("auto")


def test_minp_stepdown_and_sequential_against_the_same_labels(eng, case257):
    from oracle import oracle as orc
    from scoary_amd import tree as T_
    c = case257
    T, G, P = c.T, c.G, c.P
    res = eng.associate(c.gm, c.trv, c.mkv, permutations=P, seed=c.seed, use_lists=False, strata=c.sp, fwer=True)
    p = res["p"].cpu().numpy()
    pp = c.want_p_perm(eng, res["counts"])
    want_minp = pp.min(2)
    assert np.array_equal(res["minp"].cpu().numpy(), want_minp)
    assert np.array_equal(eng.minp(c.gm, c.trv, c.mkv, P, c.seed, strata=c.sp).cpu().numpy(), want_minp)
    want_fwer = (want_minp[:, :, None] <= p[:, None, :]).sum(1)
    assert np.array_equal(res["r_fwer"].cpu().numpy(), want_fwer)
    # step-down (spec S8): successive minima along the (p, gene index) order, ties take their first, running maximum
    r_sd, minp = eng.minp_stepdown(c.gm, c.trv, c.mkv, P, c.seed, res=res, strata=c.sp)
    assert np.array_equal(minp.cpu().numpy(), want_minp)
    want_sd = np.zeros((T, G), dtype=np.int64)
    for t in range(T):
        order = np.argsort(p[t], kind="stable")
        q = np.minimum.accumulate(pp[t][:, order][:, ::-1], axis=1)[:, ::-1]          # [P, rank]
        cnt = (q <= p[t][order][None, :]).sum(0)
        for k in range(1, G):
            if p[t][order[k]] == p[t][order[k - 1]]:
                cnt[k] = cnt[k - 1]
        want_sd[t, order] = np.maximum.accumulate(cnt)
    assert np.array_equal(r_sd.cpu().numpy(), want_sd)
    assert (want_sd <= want_fwer).all()
    # the sequential estimator with early abort
    thr = T_._abort_thresholds(P)
    r, nstop = eng.permute_sequential(c.gm, c.mkv, res["margins"], res["crit"], P, c.seed, thr, strata=c.sp)
    r, nstop = r.cpu().numpy().view(np.uint32), nstop.cpu().numpy().view(np.uint32)
    got = (r + 1.0) / (np.where(nstop > 0, nstop, P) + 1.0)
    crit = res["crit"].cpu().numpy().view(np.uint32).astype(np.int64)
    flags = ((c.a - crit[:, None, :, 0]) & 0xffffffff) >= crit[:, None, :, 1]         # [T, P, G]
    stopped = 0
    for t in range(T):
        for g in range(G):
            assert got[t, g] == orc.empirical_p_with_abort(flags[t, :, g]), (t, g)
            stopped += nstop[t, g] > 0
    assert 0 < stopped < T * G


def test_a_trait_that_is_constant_inside_every_stratum(eng):
    """The confounded case: with the trait constant in every stratum, every within-stratum shuffle is the observed
    labelling -- r = P for every gene, every minimum is the observed smallest p, the best gene's r_fwer = P.  The
    same inputs without strata give r < P for a planted lineage marker."""
    from scoary_amd.engine import pack_bits_rows
    rng = np.random.default_rng(3)
    G, N, P, S = 200, 300, 256, 6
    strata = rng.integers(0, S, N)
    trait = (strata < 3).astype(np.uint8)[None]
    genes = (rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))).astype(np.uint8)
    genes[0] = np.where(rng.random(N) < 0.95, trait[0], 1 - trait[0])               # the lineage marker
    gm = eng.pack_dense(genes)
    trv = eng.vecrows(pack_bits_rows(trait), N)
    mkv = eng.vecrows(pack_bits_rows(np.ones_like(trait)), N)
    sp = eng.strata_plan(strata, trv, mkv, N)
    res = eng.associate(gm, trv, mkv, permutations=P, seed=1, strata=sp, fwer=True, stepdown=True)
    p = res["p"].cpu().numpy()
    assert (res["r"].cpu().numpy() == P).all()
    assert (res["minp"].cpu().numpy() == p.min()).all()
    best = int(np.argmin(p[0]))
    assert best == 0 and res["r_fwer"].cpu().numpy()[0, best] == P and res["r_fwer_sd"].cpu().numpy()[0, best] == P
    plain = eng.associate(gm, trv, mkv, permutations=P, seed=1, fwer=True)
    assert plain["r"].cpu().numpy()[0, 0] < P and plain["r_fwer"].cpu().numpy()[0, 0] < P


@pytest.mark.parametrize("use_lists", [True, False], ids=["lists", "dense"])
def test_auto_graph_keeps_stratified_and_plain_steps_apart(eng, case257, use_lists):
    """One workspace, one trait plan: three calls without strata, then three with -- each set gives its own results
    (a graph recorded for one is never replayed for the other)."""
    import torch
    c = case257
    if use_lists and c.gm.lists is None:
        eng.build_lists(c.gm)
    ws = eng.workspace(c.gm, c.T, c.P, use_lists=use_lists)
    assert eng.auto_graph_eligible(c.gm, c.T, c.P)
    want_plain = eng.associate(c.gm, c.trv, c.mkv, permutations=c.P, seed=c.seed, use_lists=use_lists)
    want_plain = want_plain["r"].cpu().numpy().copy()
    want_strata = c.want_r(eng.fisher(eng.counts(c.gm, c.trv, c.mkv)[0])[2])
    assert not np.array_equal(want_plain.view(np.uint32), want_strata)
    for sp, want in ((None, want_plain.view(np.uint32)), (c.sp, want_strata), (None, want_plain.view(np.uint32))):
        for call in range(3):
            ws.r.fill_(-1)
            res = eng.associate(c.gm, c.trv, c.mkv, permutations=c.P, seed=c.seed, use_lists=use_lists,
                                workspace=ws, plan=c.plan, strata=sp)
            torch.cuda.synchronize()
            assert np.array_equal(res["r"].cpu().numpy().view(np.uint32), want), (sp is not None, call)
            assert (ws.auto["graph"] is not None) == (call >= 1)
