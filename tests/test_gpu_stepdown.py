"""Westfall-Young step-down minP (spec S8): k_stepdown_minp, the engine's permute_stepdown() / minp_stepdown() /
associate(stepdown=True) and the --permute-fwer-stepdown column, exactly against the numpy reference of the spec
over p-values from the oracle (up to 170 isolates) or the engine's own scoary_fisher (above)."""
import csv
import io
import os

import numpy as np
import pytest

from conftest import golden_text, read_dense
from test_gpu_minp import (SEED, bits, count_leq, device_inputs, observed_tables, oracle_labels, permuted_tables,
                           run_cli)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


@pytest.fixture(scope="module")
def eng():
    from scoary_amd.engine import AssociationEngine
    return AssociationEngine(0)


def make_sd_data(G, N, T, seed):
    """Genes uniform over frequencies 0.05-0.95; a block of 2G/5 genes follows trait 0 with 8-45 % of the labels
    flipped (the lineage block the step-down exists for), six exact duplicates (tied p), one absent and one core
    gene; trait 1 has missing values."""
    rng = np.random.default_rng(seed)
    genes = (rng.random((G, N)) < rng.uniform(0.05, 0.95, (G, 1))).astype(np.uint8)
    traits = np.zeros((T, N), np.uint8)
    for t in range(T):
        traits[t] = rng.random(N) < (0.5, 0.3, 0.7)[t % 3]
    K = (2 * G) // 5
    for k, rate in enumerate(np.linspace(0.08, 0.45, K)):
        genes[10 + k] = traits[0] ^ (rng.random(N) < rate)
    genes[10 + K:10 + K + 6] = genes[12:18]     # exact duplicates: tied p
    genes[3] = 0
    genes[4] = 1
    if T > 1:
        traits[1, ::29] = 2
    return genes, traits


def stepdown_reference(pperm, p):
    """Spec S8 in numpy: pperm [P][G] = the permuted p of every gene, p [G] its own.  Returns (r_sd by gene, raw
    c by rank position, c after the tie rule, order)."""
    P, G = pperm.shape
    order = np.lexsort((np.arange(G), p))
    ps = p[order]
    q = np.minimum.accumulate(pperm[:, order][:, ::-1], axis=1)[:, ::-1]
    c = (q <= ps[None, :]).sum(axis=0)
    first = np.r_[True, ps[1:] != ps[:-1]]
    c_tied = c[np.flatnonzero(first)][np.cumsum(first) - 1]
    r = np.empty(G, np.int64)
    r[order] = np.maximum.accumulate(c_tied)
    return r, c, c_tied, order


def fisher_of(tables, fisher):
    """tables (..., 4) -> fisher(table) shaped (...), every distinct table evaluated once."""
    shape = tables.shape[:-1]
    uniq, inv = np.unique(tables.reshape(-1, 4), axis=0, return_inverse=True)
    return fisher(np.ascontiguousarray(uniq))[inv.reshape(-1)].reshape(shape)


def reference(genes, traits, P, seed, fisher):
    """(p [T, G], pperm [T][P, G], per trait stepdown_reference) under the S4 labels of ``seed``."""
    tabs = permuted_tables(genes, traits, oracle_labels(traits, P, seed))
    pperm = [fisher_of(tb, fisher) for tb in tabs]
    p = fisher_of(observed_tables(genes, traits), fisher)
    return p, pperm, [stepdown_reference(pperm[t], p[t]) for t in range(traits.shape[0])]


def oracle_fisher(u):
    from oracle import oracle as orc
    return orc.fisher_many(u)[1]


def engine_fisher(eng):
    import torch

    def f(u):
        return eng.fisher(torch.from_numpy(np.ascontiguousarray(u)).to(eng.device), want_crit=False)[0].cpu().numpy()
    return f


_ORACLE_CACHE = {}


def oracle_reference(G, N, T, P, seed):
    key = (G, N, T, P, seed)
    if key not in _ORACLE_CACHE:
        genes, traits = make_sd_data(G, N, T, seed)
        p, pperm, sd = reference(genes, traits, P, SEED, oracle_fisher)
        for a in [genes, traits, p] + pperm:
            a.setflags(write=False)
        _ORACLE_CACHE[key] = (genes, traits, p, pperm, sd)
    return _ORACLE_CACHE[key]


# ---- 1. against the oracle, N <= 170 ---------------------------------------------------------------------------
@pytest.mark.parametrize("G,N,T,P,seed", [(200, 100, 2, 192, 1), (160, 170, 2, 128, 2)])
def test_stepdown_equals_the_oracle(eng, G, N, T, P, seed):
    genes, traits, p, pperm, sd = oracle_reference(G, N, T, P, seed)
    want_r = np.stack([s[0] for s in sd])
    want_minp = np.stack([pp.min(axis=1) for pp in pperm])
    want_fwer = count_leq(want_minp, p)
    # the reference itself is not vacuous: the step-down gains, the tie rule and the running maximum all act
    if (G, N) == (200, 100):
        r0, c0, c0_tied, _order = sd[0]
        assert (r0 < want_fwer[0]).sum() >= 10
        assert (c0 != c0_tied).sum() >= 1
        assert (np.maximum.accumulate(c0_tied) != c0_tied).sum() >= 1
    assert (want_r <= want_fwer).all()
    for t in range(T):
        assert want_r[t, sd[t][3][0]] == want_fwer[t, sd[t][3][0]]
    assert (want_r[:, 3] == P).all() and (want_r[:, 4] == P).all()

    gm, trv, mkv = device_inputs(eng, genes, traits)
    res = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, use_lists=False, fwer=True, stepdown=True)
    assert np.array_equal(bits(res["p"].cpu().numpy()), bits(p))
    got = res["r_fwer_sd"].cpu().numpy()
    assert got.shape == (T, G) and got.dtype == np.int32
    assert np.array_equal(got, want_r)
    alone = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, use_lists=False, fwer=True)
    assert "r_fwer_sd" not in alone
    assert np.array_equal(bits(res["minp"].cpu().numpy()), bits(alone["minp"].cpu().numpy()))
    assert np.array_equal(bits(res["minp"].cpu().numpy()), bits(want_minp))
    assert np.array_equal(res["r_fwer"].cpu().numpy(), alone["r_fwer"].cpu().numpy())
    assert np.array_equal(res["r_fwer"].cpu().numpy(), want_fwer)


# ---- 2. the kernel alone over synthetic tables: every position informative ---------------------------------------
# tiled row size (quads) of every N used below: which k_stepdown_minp instance the case reaches -- every register row
# size (1, 2, 4, 6, 8, 12, 16, 20, 24 quads) and the chunked kernel (> 24)
ROW_QUADS = {100: 1, 131: 2, 200: 2, 400: 4, 700: 6, 900: 8, 1300: 12, 1800: 16, 2300: 20, 2600: 24, 3300: 32,
             7000: 56}
# the fewest chunks of the rank order the cases that are there for the walk over several chunks must reach; those
# with N > 3072 are the chunked instances
MIN_CHUNKS = {(1100, 100, 2, 70): 3, (1100, 131, 2, 33): 3, (603, 3300, 2, 40): 3, (300, 7000, 1, 33): 2,
              (603, 3300, 1, 40): 3}


def several_chunks(eng, G, N, T, P, least):
    """Asserts that the launch shape walks the G genes / rank positions in at least ``least`` chunks with a ragged
    last one -- for the chunked instances (groups of eight) one that also ends inside a group; -> (chunks, chunk
    length)."""
    nch = eng.stepdown_chunks(G, T, P)
    gchunk = -(-(-(-G // nch)) // 64) * 64                         # a chunk is ceil(G / nch) rounded up to 64 positions
    assert nch >= least and (nch - 1) * gchunk < G and G % gchunk != 0
    if N > 3072:
        assert eng.quads(N) > 24 and (G % gchunk) % 8 != 0
    return nch, gchunk


@pytest.mark.parametrize("G,N,T,P", [(1100, 100, 2, 70), (1100, 131, 2, 33), (130, 2600, 1, 40), (130, 3300, 1, 40),
                                     (603, 3300, 2, 40), (300, 7000, 1, 33)]
                         + [(130, N, 1, 40) for N in (200, 400, 700, 900, 1300, 1800, 2300)])
def test_raw_counts_over_synthetic_tables(eng, G, N, T, P):
    """The real CSR layout of the p tables filled with random doubles, random label rows (they may leave a gene's
    support: the clamp of the gather is part of the contract), a random rank order and p_sorted drawn from the
    successive minima themselves: counts in mid-range at most positions, exact equalities, a tie run of 40.
    G = 1100 is walked in >= 3 chunks with a ragged last one (both passes); N = 131 / P = 33 are ragged at the quad
    and the lane; N = 2600 and N = 3300 are the largest register-resident row and the chunked instance; the other
    (130, N, 1, 40) cases walk the remaining register row sizes, both passes' instances of each.  (603, 3300, 2, 40)
    and (300, 7000, 1, 33) walk the chunked instance in >= 3 and >= 2 chunks whose last one ends inside a group of
    eight positions: pass A of the chunked kernel, the carry into its pass B, the rank-ordered copy of the rows read
    from a position above 0."""
    import torch
    from scoary_amd.engine import MinpTables, pack_bits_rows
    assert eng.quads(N) == ROW_QUADS[N]                 # which instance the shape reaches
    assert (eng.quads(N) > 24) == (N > 3072)
    rng = np.random.default_rng(7000 + N)
    genes, traits = make_sd_data(G, N, T, 5)
    gm, trv, mkv = device_inputs(eng, genes, traits)
    counts, _margins = eng.counts(gm, trv, mkv)
    real = eng.minp_tables(counts)
    off = real.off.cpu().numpy()
    lo = real.lo.cpu().numpy()
    for _draw in range(3):
        # a draw can come out flat: a one-entry table (the absent or the core gene) with a small p late in the rank
        # order is the minimum of every position before it.  Then the same stream is drawn from again
        tab = rng.random(real.entries)
        labels = (rng.random((T, P, N)) < rng.uniform(0.2, 0.8, (T, P, 1))).astype(np.uint8)
        order = np.stack([rng.permutation(G) for _ in range(T)]).astype(np.int32)
        ps = np.empty((T, G))
        q = []
        for t in range(T):
            a = labels[t].astype(np.int64) @ genes.T.astype(np.int64)                       # [P, G]
            size = np.diff(off)[t * G:(t + 1) * G]
            idx = np.clip(a - lo[t][None, :], 0, size[None, :] - 1)
            pperm = tab[off[t * G:(t + 1) * G][None, :] + idx]
            q.append(np.minimum.accumulate(pperm[:, order[t]][:, ::-1], axis=1)[:, ::-1])
            ps[t] = np.sort(q[t][rng.integers(0, P, G), np.arange(G)])                     # entries of tab, ascending
            a0 = 500 if G > 600 else 50
            ps[t, a0:a0 + 40] = ps[t, a0]                                                  # a run of 40 equal values
            assert (np.diff(ps[t]) >= 0).all()
        want_c = np.stack([(q[t] <= ps[t][None, :]).sum(axis=0) for t in range(T)])
        want_minp = np.stack([q[t][:, 0] for t in range(T)])
        if ((want_c > 0) & (want_c < P)).mean() > 0.5:
            break
    tables = MinpTables(real.off, real.lo, torch.from_numpy(tab).to(eng.device), real.entries)
    perms = torch.stack([eng.vecrows(pack_bits_rows(labels[t]), N) for t in range(T)]).contiguous()
    # informative: most positions strictly between 0 and P, and the exact-equality case occurs
    assert ((want_c > 0) & (want_c < P)).mean() > 0.5
    assert sum(int((q[t] == ps[t][None, :]).sum()) for t in range(T)) >= 10

    if (G, N, T, P) in MIN_CHUNKS:
        several_chunks(eng, G, N, T, P, MIN_CHUNKS[(G, N, T, P)])
    c = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    minp = torch.ones((T, P), dtype=torch.float64, device=eng.device)
    out = eng.permute_stepdown(gm, perms, tables, torch.from_numpy(order).to(eng.device),
                               torch.from_numpy(ps).to(eng.device), c, minp=minp)
    assert out is c
    assert np.array_equal(c.cpu().numpy().astype(np.int64), want_c)
    assert np.array_equal(bits(minp.cpu().numpy()), bits(want_minp))
    # batches add into c, and the minima are optional
    c2 = torch.zeros_like(c)
    half = P // 2
    eng.permute_stepdown(gm, perms[:, :half].contiguous(), tables, torch.from_numpy(order).to(eng.device),
                         torch.from_numpy(ps).to(eng.device), c2)
    eng.permute_stepdown(gm, perms[:, half:].contiguous(), tables, torch.from_numpy(order).to(eng.device),
                         torch.from_numpy(ps).to(eng.device), c2)
    assert torch.equal(c2, c)


# ---- 3. above 170 isolates, against the engine's own scoary_fisher ----------------------------------------------
@pytest.mark.parametrize("G,N,T,P", [(150, 333, 2, 96), (130, 3300, 1, 40), (603, 3300, 1, 40)])
def test_stepdown_equals_fisher_of_the_permuted_tables(eng, G, N, T, P):
    """(603, 3300, 1, 40): the chunked instance over three chunks, the last one ragged, through the whole step."""
    if (G, N, T, P) in MIN_CHUNKS:
        several_chunks(eng, G, N, T, P, MIN_CHUNKS[(G, N, T, P)])
    genes, traits = make_sd_data(G, N, T, 3)
    p, pperm, sd = reference(genes, traits, P, SEED, engine_fisher(eng))
    gm, trv, mkv = device_inputs(eng, genes, traits)
    res = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, use_lists=False, stepdown=True)
    assert "r_fwer" not in res
    assert np.array_equal(bits(res["p"].cpu().numpy()), bits(p))
    assert np.array_equal(res["r_fwer_sd"].cpu().numpy(), np.stack([s[0] for s in sd]))
    assert np.array_equal(bits(res["minp"].cpu().numpy()), bits(np.stack([pp.min(axis=1) for pp in pperm])))


# ---- 4. identity labelling over many chunks ---------------------------------------------------------------------
def test_identity_labelling_counts_every_permutation(eng):
    import torch
    G, N, T, P = 5000, 2000, 3, 70
    genes, traits = make_sd_data(G, N, T, 4)
    gm, trv, mkv = device_inputs(eng, genes, traits)
    res = eng.associate(gm, trv, mkv)
    tables = eng.minp_tables(res["counts"])
    assert eng.stepdown_chunks(G, T, P) >= 8
    perms = trv[:, None, :].expand(T, P, trv.shape[1]).contiguous()       # the observed rows as "permutations"
    ps, order = torch.sort(res["p"], dim=1, stable=True)
    c = torch.zeros((T, G), dtype=torch.int32, device=eng.device)
    minp = torch.ones((T, P), dtype=torch.float64, device=eng.device)
    eng.permute_stepdown(gm, perms, tables, order.to(torch.int32).contiguous(), ps.contiguous(), c, minp=minp)
    assert (c == P).all()
    want = res["p"].min(dim=1).values.cpu().numpy()
    assert (want < 1e-6).any()
    assert np.array_equal(bits(minp.cpu().numpy()), bits(np.repeat(want[:, None], P, axis=1)))


# ---- 5. composition ---------------------------------------------------------------------------------------------
def test_batches_trait_groups_and_cached_tables_compose(eng):
    import torch
    G, N, T, P, seed = 200, 100, 2, 192, 1
    genes, traits, _p, pperm, sd = oracle_reference(G, N, T, P, seed)
    gm, trv, mkv = device_inputs(eng, genes, traits)
    r_whole, m_whole = eng.minp_stepdown(gm, trv, mkv, P, SEED)
    assert np.array_equal(r_whole.cpu().numpy(), np.stack([s[0] for s in sd]))
    assert np.array_equal(bits(m_whole.cpu().numpy()), bits(np.stack([pp.min(axis=1) for pp in pperm])))

    def same(got):
        return torch.equal(got[0], r_whole) and torch.equal(got[1].view(torch.int64), m_whole.view(torch.int64))
    # label rows in batches of 50 permutations
    assert same(eng.minp_stepdown(gm, trv, mkv, P, SEED, label_budget_bytes=50 * T * eng.row_words(N) * 4))
    # one trait per table group
    counts, _m = eng.counts(gm, trv, mkv)
    assert eng.minp_trait_groups(counts, 1) == [(0, 1), (1, 2)]
    assert same(eng.minp_stepdown(gm, trv, mkv, P, SEED, table_budget_bytes=1))
    # with a trait plan the tables stay with the gene matrix and are reused -- by minp() as well
    assert gm.minp_cache is None
    plan = eng.trait_plan(trv, mkv, N)
    assert same(eng.minp_stepdown(gm, trv, mkv, P, SEED, plan=plan))
    kept = gm.minp_cache["tables"]
    assert same(eng.minp_stepdown(gm, trv, mkv, P, SEED, plan=plan))
    assert gm.minp_cache["tables"] is kept
    assert torch.equal(eng.minp(gm, trv, mkv, P, SEED, plan=plan).view(torch.int64), m_whole.view(torch.int64))
    assert gm.minp_cache["tables"] is kept


# ---- 6. command line --------------------------------------------------------------------------------------------
def test_cli_permute_fwer_stepdown_column(exampledir, tmp_path):
    P, seed = 100, 1234
    inputs = ["-g", os.path.join(exampledir, "Gene_presence_absence.csv"),
              "-t", os.path.join(exampledir, "Tetracycline_resistance.csv")]
    common = inputs + ["--no_pairwise", "-e", str(P), "--seed", str(seed), "-p", "1.0"]
    plain = run_cli(common, tmp_path / "plain")
    stepdown = run_cli(common + ["--permute-fwer-stepdown"], tmp_path / "stepdown")
    fwer = run_cli(common + ["--permute-fwer"], tmp_path / "fwer")
    both = run_cli(common + ["--permute-fwer", "--permute-fwer-stepdown"], tmp_path / "both")
    ids, strains, genes, names, traits = read_dense(
        golden_text("exampledata/Gene_presence_absence.csv.gz"),
        golden_text("exampledata/Tetracycline_resistance.csv.gz"))
    assert len(strains) == 100
    _p, _pperm, sd = reference(genes, traits, P, seed, oracle_fisher)
    for t, trait in enumerate(names):
        fn = trait + ".results.csv"
        r_sd = sd[t][0]
        rows = list(csv.reader(io.StringIO(stepdown[fn])))
        assert rows[0][13:] == ["Empirical_p", "Westfall_Young_stepdown_p"]
        assert len(rows) > 10
        for d in rows[1:]:
            want = (float(r_sd[ids.index(d[0])]) + 1.0) / (P + 1.0)
            assert d[14] == repr(want), (trait, d[0], d[14], want)
        stripped = "".join(line.rsplit(",", 1)[0] + "\n" for line in stepdown[fn].splitlines())
        assert stripped == plain[fn]
        assert "Westfall_Young" not in plain[fn]
        rows2 = list(csv.reader(io.StringIO(both[fn])))
        assert rows2[0][13:] == ["Empirical_p", "Westfall_Young_p", "Westfall_Young_stepdown_p"] and len(rows2[0]) == 16
        assert [r[15] for r in rows2] == [r[14] for r in rows]
        stripped2 = "".join(line.rsplit(",", 1)[0] + "\n" for line in both[fn].splitlines())
        assert stripped2 == fwer[fn]                    # the Westfall_Young_p cells of --permute-fwer alone, in bytes
