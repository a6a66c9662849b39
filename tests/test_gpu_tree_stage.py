"""The kernels of scoary_tree.hip past their easy shapes: the exceedance epilogue of
k_tree_dp<true> with many genes, a pruned tree and batched permutations; the --collapse hash
(k_row_hash) as a partition over several quads, blocks and masks; the device UPGMA loop past
one stride of its reductions.  References: the oracle, Python integers, numpy."""
from types import SimpleNamespace

import numpy as np
import pytest

import tree_stage_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from scoary_amd.engine import AssociationEngine
    e = AssociationEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# ------------------------------------------------------------------ A: exceedance flags ----
@pytest.fixture(scope="module")
def exceed_refs(orc):
    """The five cases with the oracle's results (host only).  That they reach every branch of
    the epilogue is test_host_logic.test_tree_exceed_inputs_meet_every_branch."""
    return tc.exceed_references(orc)


@pytest.mark.parametrize("k", range(len(tc.EXCEED_CASES)), ids=["K%d" % K for K, _ in tc.EXCEED_CASES])
def test_exceed_flags_vs_oracle_and_exact_integers(eng, exceed_refs, k):
    """scoary_tree_permute through methods._TreeStage -- 39 genes x 50 permutations of trait 3
    on a tree pruned of five isolates, in batches of 13, 13, 13 and 11 permutations -- equals
    (1) the oracle gene by gene, every flag, and (2) the exact-integer predicate on the
    device's own (total, pro, anti) triples under the regenerated labels."""
    from scoary_amd import methods as m, tree as T
    from scoary_amd.engine import pack_bits_rows
    c = exceed_refs[k]
    G, P = tc.EXCEED_GENES, tc.EXCEED_PERMS
    missing = [c.names[i] for i in np.nonzero(c.trait == 2)[0]]
    ptree = T.prune_missing(c.tree, missing + [None])
    assert tc.same_tree(ptree, c.ptree)
    stage = m._TreeStage(eng, ptree, c.names, c.trait, tc.EXCEED_TRAIT_INDEX, tc.EXCEED_LABEL_SEED)
    assert stage.prog.ntips == c.K < c.N
    rows = pack_bits_rows(c.genes)
    obs = stage.observed(rows)
    assert np.array_equal(obs, c.obs)
    ex = stage.permute(rows, obs, P, batch_threads=G * 13)
    assert ex.shape == (G, P) and ex.dtype == np.uint8
    assert stage.permute(rows, obs, P).tobytes() == ex.tobytes()        # one batch == four batches
    # reference 1: the oracle's program, labels and fp64 comparison
    bad = np.argwhere(ex != c.flags)
    assert len(bad) == 0, (c.K, bad[:5].tolist())
    # reference 2: same labels, exact integers
    perms = eng.perm_generate(stage.mask_rows, stage.margins, c.N, P, 0, tc.EXCEED_LABEL_SEED,
                              trait_base=tc.EXCEED_TRAIT_INDEX)
    ptip = eng.gather_bits(perms[0], stage.tips)
    pairs = eng.tree_pairs(stage.ops, stage.prog.depth, stage._gene_tip_bits(rows), ptip,
                           stage.prog.ntips).cpu().numpy()
    assert np.array_equal(pairs, c.pairs)
    want, ties = tc.exact_exceed(obs, pairs)
    bad = np.argwhere(ex != want)
    assert len(bad) == 0, (c.K, bad[:5].tolist())
    assert ties.any() and ex[ties].all()                                # the >= boundary, on the device's triples
    assert not ex[-2:].any()                                            # observed total 0: est is 0/0


# ------------------------------------------------------------------ B: --collapse hash ----
@pytest.mark.parametrize("N", tc.HASH_SIZES)
def test_row_hash_classes_equal_masked_row_classes(eng, N):
    """Two genes share a 128-bit hash <=> their rows ANDed with the trait's validity row are
    equal: partitions are compared, never hash values.  A false split (a missed mask word, a
    stale padding word, the last quad) and a false merge (a missed row word) each break it."""
    from scoary_amd.engine import pack_bits_rows
    c = tc.hash_case(N)
    G, S = c.genes.shape[0], N + 1
    h = eng.row_hash(eng.pack_dense(c.genes), eng.vecrows(pack_bits_rows(c.valid), N))
    assert h.shape == (3, G, 2)
    for t in range(3):
        masked = c.genes & c.valid[t][None, :]
        want = np.unique(masked, axis=0, return_inverse=True)[1]
        got = np.unique(h[t], axis=0, return_inverse=True)[1]
        assert np.array_equal(tc.first_seen_ids(got), tc.first_seen_ids(want)), (N, t)
        assert np.array_equal(h[t, G - 3:], h[t, c.copied]), (N, t)     # the copies, across blocks

    def classes(t):
        return tc.first_seen_ids(np.unique(h[t, c.sweep], axis=0, return_inverse=True)[1])
    # all valid: base and its N single-bit neighbours are all distinct
    assert classes(0).max() + 1 == S
    # some missing: exactly the rows flipped at a missing isolate fall into the base's class
    same_as_base = np.nonzero(classes(1) == 0)[0]
    assert same_as_base.tolist() == [0] + (1 + np.nonzero(c.valid[1] == 0)[0]).tolist()
    assert classes(1).max() + 1 == 1 + int(c.valid[1].sum())
    # one valid isolate: the row flipped there, and everything else
    assert classes(2).max() + 1 <= 2


def test_pattern_groups_same_with_and_without_device_hashes(eng):
    """methods._pattern_groups -- the way a false split would reach a results file -- gives the
    same groups from the device hashes as from the bit rows alone (group ids are arbitrary
    labels: compared by order of first appearance)."""
    from scoary_amd import methods as m
    from scoary_amd.engine import pack_bits_rows
    N = 257
    c = tc.hash_case(N)
    G = c.genes.shape[0]
    h = eng.row_hash(eng.pack_dense(c.genes), eng.vecrows(pack_bits_rows(c.valid), N))
    table = SimpleNamespace(rows64=pack_bits_rows(c.genes))
    idx = np.delete(np.arange(G), [2, 100, G - 2])                       # "testable" genes: a strict subset
    for t in range(3):
        maskrow = pack_bits_rows(c.valid[t:t + 1])[0]
        with_h = m._pattern_groups(table, maskrow, idx, h[t])
        without = m._pattern_groups(table, maskrow, idx, None)
        assert np.array_equal(tc.first_seen_ids(with_h), tc.first_seen_ids(without)), t
        masked = (c.genes & c.valid[t][None, :])[idx]
        want = np.unique(masked, axis=0, return_inverse=True)[1]
        assert np.array_equal(tc.first_seen_ids(with_h), tc.first_seen_ids(want)), t


# ------------------------------------------------------------------ C: device UPGMA ----
@pytest.mark.parametrize("n", sorted(tc.UPGMA_CASES))
def test_device_upgma_past_one_stride(eng, n):
    """scoary_upgma == the numpy quad-tree loop with more than 1024 isolates: every 1024-stride
    loop of k_upgma_merge and every 256-stride scan of k_upgma_rowmin takes more than one turn,
    and the Morton tie order compares indices that differ above bit 8 (1300: duplicated strains).
    At 1280 the first merges are between rows that only the second turn of the minimum reduction
    reads (tree_stage_cases.upgma_case says why 1025 and 1300 cannot show that)."""
    from scoary_amd import tree as T
    var, names, cnt = tc.upgma_case(n)
    want = T.upgma_from_counts(cnt, var.shape[1], names, native=False)
    merges = eng.upgma_merges(var)
    assert merges is not None                             # the device loop ran, not the fallback
    assert merges.shape == (n - 1, 2)
    cluster = list(names)
    for i, j in merges.tolist():
        assert cluster[i] is not None and cluster[j] is not None and i != j
        cluster[i], cluster[j] = [cluster[i], cluster[j]], None
    assert tc.same_tree(cluster[i], want)
    assert tc.same_tree(T.upgma(eng, var.T, names), want)
