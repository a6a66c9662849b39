"""Westfall-Young single-step minP (spec S7): the p tables, k_permute_minp, the engine's minp() /
associate(fwer=True) and the --permute-fwer column, bit for bit against a reference composed from the
oracle's own exports (perm_labels, pack_rows, fisher_many) and numpy."""
import csv
import io
import os
import sys

import numpy as np
import pytest

from conftest import golden_text, read_dense

pytestmark = pytest.mark.gpu

SEED = 4242


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


@pytest.fixture(scope="module")
def eng():
    from scoary_amd.engine import AssociationEngine
    return AssociationEngine(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_data(G, N, T, rng_seed):
    """Genes uniform over frequencies 0.02-0.98 plus one absent and one core gene; trait 0 planted on a gene
    with 10 % of its labels flipped, trait 1 with missing values (and, when there are only two traits, the
    ~70 % positives), trait 2 with ~70 % positives: supports that start above 0."""
    rng = np.random.default_rng(rng_seed)
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    genes[3] = 0
    genes[4] = 1
    traits = np.zeros((T, N), dtype=np.uint8)
    planted = genes[7].copy()
    flip = rng.random(N) < 0.10
    planted[flip] ^= 1
    traits[0] = planted
    if T > 1:
        traits[1] = rng.random(N) < (0.7 if T == 2 else 0.4)
        traits[1, ::29] = 2
    for t in range(2, T):
        traits[t] = rng.random(N) < 0.7
    return genes, traits


def oracle_labels(traits, P, seed, trait_base=0):
    """[T][P, N] 0/1 label rows of spec S4 from the oracle's generator."""
    from oracle import oracle as orc
    T, N = traits.shape
    out = []
    for t in range(T):
        mask_bits = orc.pack_rows((traits[t:t + 1] != 2).astype(np.uint8))[0]
        npos = int((traits[t] == 1).sum())
        rows = np.stack([orc.perm_labels(seed, trait_base + t, pi, mask_bits, npos, N) for pi in range(P)])
        out.append(np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :N])
    return out


def permuted_tables(genes, traits, labels):
    """[T] int32 arrays (P, G, 4): the table of every gene under every permuted labelling, by numpy."""
    out = []
    for t, lab in enumerate(labels):
        valid = traits[t] != 2
        npos, nval = int((traits[t] == 1).sum()), int(valid.sum())
        gm = genes[:, valid].astype(np.int64).sum(axis=1)[None, :]
        a = lab.astype(np.int64) @ genes.T.astype(np.int64)
        out.append(np.stack([a, npos - a, gm - a, nval - npos - gm + a], axis=2).astype(np.int32))
    return out


def observed_tables(genes, traits):
    from oracle import oracle as orc
    from scoary_amd.engine import pack_bits_rows
    return orc.counts_packed(orc.pack_rows(genes), pack_bits_rows((traits == 1).astype(np.uint8)),
                             pack_bits_rows((traits != 2).astype(np.uint8))).transpose(1, 0, 2)


def min_over_genes(tables, fisher):
    """tables (P, G, 4) -> min over genes of fisher(table), every distinct table evaluated once."""
    P, G, _ = tables.shape
    uniq, inv = np.unique(tables.reshape(-1, 4), axis=0, return_inverse=True)
    return fisher(uniq)[inv.reshape(-1)].reshape(P, G).min(axis=1)


def count_leq(minp, p):
    return (minp[:, :, None] <= p[:, None, :]).sum(axis=1).astype(np.int32)


def device_inputs(eng, genes, traits):
    from scoary_amd.engine import pack_bits_rows
    N = genes.shape[1]
    gm = eng.pack_dense(np.array(genes))            # a writable copy: the shared reference arrays are read-only
    trv = eng.vecrows(pack_bits_rows((traits == 1).astype(np.uint8)), N)
    mkv = eng.vecrows(pack_bits_rows((traits != 2).astype(np.uint8)), N)
    return gm, trv, mkv


_ORACLE_CACHE = {}


def oracle_reference(G, N, T, P):
    """(genes, traits, minp [T, P], p [T, G], r_fwer [T, G]) by the oracle, computed once per shape."""
    key = (G, N, T, P)
    if key not in _ORACLE_CACHE:
        from oracle import oracle as orc
        genes, traits = make_data(G, N, T, 1000 + N)
        tabs = permuted_tables(genes, traits, oracle_labels(traits, P, SEED))
        minp = np.stack([min_over_genes(tb, lambda u: orc.fisher_many(u)[1]) for tb in tabs])
        p = orc.fisher_many(observed_tables(genes, traits).reshape(-1, 4))[1].reshape(T, G)
        for a in (genes, traits, minp, p):
            a.setflags(write=False)
        _ORACLE_CACHE[key] = (genes, traits, minp, p, count_leq(minp, p))
    return _ORACLE_CACHE[key]


# ---- 1. bit-exact against the oracle, N <= 170 ------------------------------------------------------------------
@pytest.mark.parametrize("G,N,T,P", [(300, 100, 3, 256), (200, 170, 2, 128)])
def test_minp_bits_equal_the_oracle(eng, G, N, T, P):
    """Up to 170 isolates both sides return SciPy's own double: minp and r_fwer are demanded bit for bit (the
    oracle itself has exact ties minp == p_g and pairs closer than 1e-11: a tolerance could not tell them apart)."""
    genes, traits, want_minp, want_p, want_r = oracle_reference(G, N, T, P)
    gm, trv, mkv = device_inputs(eng, genes, traits)
    res = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, use_lists=False, fwer=True)
    got_minp = res["minp"].cpu().numpy()
    got_r = res["r_fwer"].cpu().numpy()
    assert got_minp.shape == (T, P) and got_r.shape == (T, G)
    assert np.array_equal(bits(res["p"].cpu().numpy()), bits(want_p))
    assert np.array_equal(bits(got_minp), bits(want_minp))
    assert np.array_equal(got_r, want_r)
    # a non-trivial mix: some gene below every minimum, some strictly in between, untested genes at P
    # (the planted trait has a gene with r_fwer = 0, every trait has several genes strictly between 0 and P)
    assert (want_r[0] == 0).any()
    for t in range(T):
        assert ((want_r[t] > 0) & (want_r[t] < P)).sum() >= 5 and (want_r[t] == P).sum() > G // 2
    assert (want_r[:, 3] == P).all() and (want_r[:, 4] == P).all()


# ---- 2. bit-exact above 170 (and at the ragged edges), against the engine's own scoary_fisher --------------------
# tiled row size (quads) of every N used below: which k_permute_minp instance the case reaches.  With 100 (test 1) the
# cases cover every register row size -- 1, 2, 4, 6, 8, 12, 16, 20, 24 quads -- and the chunked kernel (> 24); 2000 is
# test_gpu_wy_scale.py's
ROW_QUADS = {100: 1, 131: 2, 200: 2, 333: 4, 400: 4, 700: 6, 900: 8, 1300: 12, 1800: 16, 2000: 16, 2300: 20, 2600: 24,
             3300: 32, 7000: 56}


@pytest.mark.parametrize("G,N,T,P", [(150, 333, 2, 96), (130, 2600, 1, 40), (70, 131, 2, 33), (130, 3300, 1, 40),
                                     (70, 7000, 2, 33), (603, 3300, 2, 40), (300, 7000, 1, 33)]
                         + [(70, N, 1, 33) for N in (200, 400, 700, 900, 1300, 1800, 2300)])
def test_minp_bits_equal_fisher_of_the_permuted_tables(eng, G, N, T, P):
    """Tables from the oracle's labels and numpy counts, pushed through eng.fisher: the minimum per (trait,
    permutation) must be minp bit for bit.  N = 2600 is the largest register-resident instance (24 quads, up to 3072
    isolates); N = 3300 and N = 7000 (32 and 56 quads) run k_permute_minp_chunked; N = 131 / P = 33 / G = 70 are
    ragged at the quad, lane and block edges; the (70, N, 1, 33) cases walk the remaining register row sizes: a wrong
    instance reads the label rows at the wrong stride.  G = 603 and G = 300 give k_permute_minp_chunked several gene
    chunks: blocks that start at a gene above 0, and a last chunk that ends inside a pass of eight genes."""
    assert eng.quads(N) == ROW_QUADS[N]                 # which instance the shape reaches
    assert (eng.quads(N) > 24) == (N > 3072)            # ... of which kernel
    if G > 256:
        # the launch shape is the step-down's (one function of the library serves both entry points)
        nch = eng.stepdown_chunks(G, T, P)
        gchunk = -(-(-(-G // nch)) // 64) * 64          # a chunk is ceil(G / nch) rounded up to 64 genes
        assert eng.quads(N) > 24 and nch > 1 and (nch - 1) * gchunk < G and (G % gchunk) % 8 != 0
    import torch
    genes, traits = make_data(G, N, T, 2000 + N)
    tabs = permuted_tables(genes, traits, oracle_labels(traits, P, SEED))

    def dev_fisher(u):
        return eng.fisher(torch.from_numpy(np.ascontiguousarray(u)).to(eng.device), want_crit=False)[0].cpu().numpy()
    want_minp = np.stack([min_over_genes(tb, dev_fisher) for tb in tabs])
    gm, trv, mkv = device_inputs(eng, genes, traits)
    res = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, use_lists=False, fwer=True)
    assert np.array_equal(bits(res["minp"].cpu().numpy()), bits(want_minp))
    assert np.array_equal(res["r_fwer"].cpu().numpy(), count_leq(want_minp, res["p"].cpu().numpy()))


# ---- 3. the table entries are scoary_fisher's --------------------------------------------------------------------
@pytest.mark.parametrize("N", [120, 700])
def test_table_entries_equal_fisher(eng, N):
    import torch
    G, T = 40, 2
    genes, traits = make_data(G, N, T, 3000 + N)
    gm, trv, mkv = device_inputs(eng, genes, traits)
    counts, _margins = eng.counts(gm, trv, mkv)
    tables = eng.minp_tables(counts)
    c = counts.cpu().numpy().astype(np.int64).reshape(-1, 4)
    npos, gmar, nval = c[:, 0] + c[:, 1], c[:, 0] + c[:, 2], c.sum(axis=1)
    lo, hi = np.maximum(0, npos + gmar - nval), np.minimum(npos, gmar)
    off = np.concatenate([[0], np.cumsum(hi - lo + 1)])
    assert np.array_equal(tables.off.cpu().numpy(), off)
    assert np.array_equal(tables.lo.cpu().numpy().reshape(-1), lo)
    assert tables.entries == off[-1] and tables.tab.numel() == off[-1]
    rows = []
    for i in range(T * G):
        a = np.arange(lo[i], hi[i] + 1)
        rows.append(np.stack([a, npos[i] - a, gmar[i] - a, nval[i] - npos[i] - gmar[i] + a], axis=1))
    enum = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(eng.device)
    want = eng.fisher(enum, want_crit=False)[0].cpu().numpy()
    assert np.array_equal(bits(tables.tab.cpu().numpy()), bits(want))


# ---- 4. identity labelling: many blocks, the atomic path ---------------------------------------------------------
def test_identity_labelling_gives_the_smallest_observed_p(eng):
    import torch
    G, N, T, P = 5000, 2000, 3, 70
    genes, traits = make_data(G, N, T, 4000)
    gm, trv, mkv = device_inputs(eng, genes, traits)
    res = eng.associate(gm, trv, mkv)
    tables = eng.minp_tables(res["counts"])
    perms = trv[:, None, :].expand(T, P, trv.shape[1]).contiguous()       # the observed rows as "permutations"
    minp = torch.ones((T, P), dtype=torch.float64, device=eng.device)
    eng.permute_minp(gm, perms, tables, minp)
    want = res["p"].min(dim=1).values.cpu().numpy()
    got = minp.cpu().numpy()
    assert (want < 1e-6).any()
    assert np.array_equal(bits(got), bits(np.repeat(want[:, None], P, axis=1)))


# ---- 5. composition ----------------------------------------------------------------------------------------------
def test_shards_batches_and_trait_groups_compose(eng):
    import torch
    from scoary_amd.dist import GenePartition
    G, N, T, P = 300, 100, 3, 256
    genes, traits, want_minp, _p, _r = oracle_reference(G, N, T, P)
    gm, trv, mkv = device_inputs(eng, genes, traits)
    whole = eng.minp(gm, trv, mkv, P, SEED)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(want_minp))
    # two stride shards of the genes, run separately and min-combined
    part = GenePartition(G, 2)
    shards = [eng.minp(eng.pack_dense(np.ascontiguousarray(genes[part.index(r)])), trv, mkv, P, SEED)
              for r in range(2)]
    assert torch.equal(torch.minimum(shards[0], shards[1]).view(torch.int64), whole.view(torch.int64))
    assert not torch.equal(shards[0], whole) and not torch.equal(shards[1], whole)
    # ... or accumulated into one buffer, as the call composes
    acc = eng.minp(eng.pack_dense(np.ascontiguousarray(genes[part.index(0)])), trv, mkv, P, SEED)
    eng.minp(eng.pack_dense(np.ascontiguousarray(genes[part.index(1)])), trv, mkv, P, SEED, out=acc)
    assert torch.equal(acc.view(torch.int64), whole.view(torch.int64))
    # ... or each shard through westfall_young(), the other shard's minima entering by ``reduce``: minp and r_fwer are
    # those of the whole matrix at the shard's genes
    full = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, fwer=True)["r_fwer"]
    for r in range(2):
        sg = eng.pack_dense(np.ascontiguousarray(genes[part.index(r)]))
        res = eng.associate(sg, trv, mkv, permutations=P, seed=SEED)
        wy = eng.westfall_young(sg, trv, mkv, P, SEED, res, fwer=True,
                                reduce=lambda m, other=shards[1 - r]: torch.minimum(m, other))
        assert sorted(wy) == ["minp", "r_fwer"]
        assert torch.equal(wy["minp"].view(torch.int64), whole.view(torch.int64))
        assert torch.equal(wy["r_fwer"], full[:, part.index(r)])
    # two permutation batches (the second starts inside a group of 64 and a Philox block of 32)
    two = eng.minp(gm, trv, mkv, P, SEED, perm_range=(0, 100))
    assert (two[:, 100:] == 1.0).all()
    eng.minp(gm, trv, mkv, P, SEED, perm_range=(100, P), out=two)
    assert torch.equal(two.view(torch.int64), whole.view(torch.int64))
    # label rows in batches of 50 permutations
    small = eng.minp(gm, trv, mkv, P, SEED, label_budget_bytes=50 * T * eng.row_words(N) * 4)
    assert torch.equal(small.view(torch.int64), whole.view(torch.int64))
    # a table budget that forces one trait per group
    counts, _m = eng.counts(gm, trv, mkv)
    assert eng.minp_trait_groups(counts, 1) == [(0, 1), (1, 2), (2, 3)]
    assert eng.minp_trait_groups(counts, 8 << 30) == [(0, 3)]
    grouped = eng.minp(gm, trv, mkv, P, SEED, table_budget_bytes=1)
    assert torch.equal(grouped.view(torch.int64), whole.view(torch.int64))
    # with a trait plan the tables stay with the gene matrix and are reused; another plan rebuilds them
    assert gm.minp_cache is None
    plan = eng.trait_plan(trv, mkv, N)
    first = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, plan=plan, fwer=True)["minp"]
    kept = gm.minp_cache["tables"]
    again = eng.associate(gm, trv, mkv, permutations=P, seed=SEED, plan=plan, fwer=True)["minp"]
    assert gm.minp_cache["tables"] is kept
    assert torch.equal(first.view(torch.int64), whole.view(torch.int64))
    assert torch.equal(again.view(torch.int64), whole.view(torch.int64))
    eng.minp(gm, trv, mkv, P, SEED, plan=eng.trait_plan(trv, mkv, N))
    assert gm.minp_cache["tables"] is not kept
    eng.minp(gm, trv, mkv, P, SEED, plan=gm.minp_cache["plan"], table_budget_bytes=1)     # three groups: nothing kept
    assert gm.minp_cache is None


# ---- 6. command line ----------------------------------------------------------------------------------------------
def run_cli(argv, outdir):
    from scoary_amd import methods as m
    old = sys.argv
    sys.argv = ["scoary"] + argv + ["-o", str(outdir), "--no-time"]
    try:
        with pytest.raises(SystemExit) as e:
            m.main()
        assert e.value.code in (0, None), e.value.code
    finally:
        sys.argv = old
    out = {}
    for fn in sorted(os.listdir(outdir)):
        if fn.endswith(".results.csv"):
            with open(os.path.join(outdir, fn), newline="") as f:
                out[fn] = f.read()
    return out


def test_cli_permute_fwer_column(exampledir, tmp_path):
    """--permute-fwer appends Westfall_Young_p after Empirical_p, = (r_fwer + 1) / (P + 1) with r_fwer from the
    oracle; without the flag the files are what they were: the same bytes as the flagged run minus its last
    column, and the reference's golden columns."""
    from oracle import oracle as orc
    P, seed = 100, 1234
    inputs = ["-g", os.path.join(exampledir, "Gene_presence_absence.csv"),
              "-t", os.path.join(exampledir, "Tetracycline_resistance.csv")]
    common = inputs + ["--no_pairwise", "-e", str(P), "--seed", str(seed), "-p", "1.0"]
    plain = run_cli(common, tmp_path / "plain")
    fwer = run_cli(common + ["--permute-fwer"], tmp_path / "fwer")
    ids, strains, genes, names, traits = read_dense(
        golden_text("exampledata/Gene_presence_absence.csv.gz"),
        golden_text("exampledata/Tetracycline_resistance.csv.gz"))
    assert len(strains) == 100
    T, G = traits.shape[0], genes.shape[0]
    tabs = permuted_tables(genes, traits, oracle_labels(traits, P, seed))
    minp = np.stack([min_over_genes(tb, lambda u: orc.fisher_many(u)[1]) for tb in tabs])
    p = orc.fisher_many(observed_tables(genes, traits).reshape(-1, 4))[1].reshape(T, G)
    r_fwer = count_leq(minp, p)
    for t, trait in enumerate(names):
        fn = trait + ".results.csv"
        rows = list(csv.reader(io.StringIO(fwer[fn])))
        assert rows[0][13] == "Empirical_p" and rows[0][14] == "Westfall_Young_p" and len(rows[0]) == 15
        assert len(rows) > 10
        for d in rows[1:]:
            want = (float(r_fwer[t, ids.index(d[0])]) + 1.0) / (P + 1.0)
            assert d[14] == repr(want), (trait, d[0], d[14], want)
        # without the flag: the flagged file minus its last column, byte for byte
        stripped = "".join(line.rsplit(",", 1)[0] + "\n" for line in fwer[fn].splitlines())
        assert stripped == plain[fn]
        assert "Westfall_Young_p" not in plain[fn]
        # ... and the reference's own columns (the golden of the same run without permutations)
        gold = list(csv.reader(io.StringIO(golden_text(os.path.join("csv_no_pairwise", fn + ".gz")))))
        mine = list(csv.reader(io.StringIO(plain[fn])))
        assert mine[0][:13] == gold[0] and len(mine) == len(gold)
        by_gene = {r[0]: r for r in mine[1:]}
        for gr in gold[1:]:
            assert by_gene[gr[0]][:10] == gr[:10]
            for a, b in zip(by_gene[gr[0]][10:13], gr[10:13]):
                assert a == b or abs(float(a) - float(b)) <= 1e-11 * abs(float(b)) + 1e-300


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_cli_permute_fwer_two_ranks_share_the_gpu(exampledir, tmp_path):
    """--permute-fwer under torch.distributed.run with two ranks on the one GPU (gloo): every rank takes the minima
    over its own stride shard, one all_reduce(MIN) of the [T, P] doubles follows, r_fwer travels in the records'
    nstop word -- and the result files are the single-process run's bytes."""
    import subprocess
    from conftest import ROOT
    inputs = ["-g", os.path.join(exampledir, "Gene_presence_absence.csv"),
              "-t", os.path.join(exampledir, "Tetracycline_resistance.csv")]
    flags = ["--no_pairwise", "-e", "100", "--seed", "1234", "-p", "1.0", "--permute-fwer"]
    one = run_cli(inputs + flags, tmp_path / "one")
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""), SCOARY_SHARE_GPU="1",
               SCOARY_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    two = tmp_path / "two"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                          "-m", "scoary_amd"] + inputs + flags + ["--no-time", "-o", str(two)],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert len(one) == 2
    for fn, text in one.items():
        assert "Westfall_Young_p" in text.splitlines()[0]
        with open(two / fn, newline="") as f:
            assert f.read() == text, fn
