"""Inputs and CPU references of the tree-stage tests (test_gpu_tree.py, test_gpu_tree_stage.py,
test_host_logic.py): random trees, the exceedance cases with their oracle results, the
--collapse hash tables and the UPGMA inputs past one stride of the device loops.  Plain
numpy and the oracle; nothing here touches the GPU."""
import sys
from types import SimpleNamespace

import numpy as np


def rand_tree(rng, tips, cat):
    """Random binary tree over ``tips`` as nested two-element lists; ``cat`` is the share of
    nodes that split off a single tip (1.0 = a caterpillar)."""
    if len(tips) == 1:
        return tips[0]
    k = 1 if rng.random() < cat else int(rng.integers(1, len(tips)))
    return [rand_tree(rng, tips[:k], cat), rand_tree(rng, tips[k:], cat)]


def same_tree(a, b):
    """a == b for nested lists, without recursion (UPGMA trees can be thousands deep)."""
    stack = [(a, b)]
    while stack:
        x, y = stack.pop()
        xl, yl = isinstance(x, list), isinstance(y, list)
        if xl != yl:
            return False
        if not xl:
            if x != y:
                return False
        elif len(x) != len(y):
            return False
        else:
            stack.extend(zip(x, y))
    return True


def first_seen_ids(labels):
    """Relabel a partition by order of first appearance: equal partitions <=> equal arrays."""
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv.reshape(-1)]


# ---------------------------------------------------------------------------------------------
# A: exceedance flags of the tree-statistic permutations
# ---------------------------------------------------------------------------------------------
EXCEED_CASES = [(2, 0), (9, 0.2), (64, 0.5), (333, 0.9), (700, 0.1)]     # (tips K, caterpillar share)
EXCEED_MISSING = 5              # isolates with a missing trait value: N = K + 5, pruned from the tree
EXCEED_GENES = 39               # 37 random rows + all absent + all present
EXCEED_PERMS = 50               # 39 x 50 = 1950 threads: the last wavefront is partly live
EXCEED_TRAIT_INDEX = 3
EXCEED_LABEL_SEED = 20231       # seed of the label permutations (spec S4)
EXCEED_DRAW_SEED = 2            # seed of the inputs; meets exceed_conditions() over the five cases, and the
                                # two-tip tree has genes with an observed pair


def exceed_case(K, cat, draw_seed=EXCEED_DRAW_SEED):
    """Tree over N = K + 5 isolates, a trait with five missing values, 39 gene rows."""
    rng = np.random.default_rng([draw_seed, K])
    N = K + EXCEED_MISSING
    names = ["t%d" % i for i in range(N)]
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        tree = rand_tree(rng, names, cat)
    finally:
        sys.setrecursionlimit(old)
    trait = (rng.random(N) < rng.uniform(0.3, 0.7)).astype(np.uint8)
    trait[rng.choice(N, EXCEED_MISSING, replace=False)] = 2
    genes = np.zeros((EXCEED_GENES, N), dtype=np.uint8)
    genes[:-2] = rng.random((EXCEED_GENES - 2, N)) < rng.uniform(0.05, 0.95, (EXCEED_GENES - 2, 1))
    genes[-1] = 1                                                        # rows -2 / -1: observed total 0
    return SimpleNamespace(K=K, N=N, names=names, tree=tree, trait=trait, genes=genes)


def exact_exceed(obs, pairs):
    """The exceedance predicate of Permute (methods.py:1353-1355) in Python integers:
    flag = (ot > 0 and bt > 0 and x * ot >= o * bt), (x, o) the supporting pair if
    obs_pro >= obs_anti, else the opposing pair.  Every count is below 2^15, so the fp64
    quotients x / bt and o / ot compare as the cross products do: rounding is monotone (keeps
    >=), and two unequal ratios differ by more than 2^-30, far above an ulp (keeps <).
    Returns (flags, exact ties) as (G, P) arrays."""
    obs, pairs = np.asarray(obs).tolist(), np.asarray(pairs).tolist()
    G, P = len(pairs), len(pairs[0])
    flags = np.zeros((G, P), dtype=np.uint8)
    ties = np.zeros((G, P), dtype=bool)
    for g in range(G):
        ot, opro, oanti = obs[g]
        side = 1 if opro >= oanti else 2
        o = obs[g][side]
        for p in range(P):
            bt, x = pairs[g][p][0], pairs[g][p][side]
            flags[g, p] = 1 if (ot > 0 and bt > 0 and x * ot >= o * bt) else 0
            ties[g, p] = ot > 0 and bt > 0 and x * ot == o * bt
    return flags, ties


def exceed_reference(orc, case):
    """The oracle's view of ``case``: its own pruning and its own stack program (another
    dialect: push / merge only, no heavy-child reordering), observed triples, exceedance flags
    of every gene, and the (total, pro, anti) triple of every (gene, permutation)."""
    N, G, P = case.N, EXCEED_GENES, EXCEED_PERMS
    index_of = {s: i for i, s in enumerate(case.names)}
    missing = [case.names[i] for i in np.nonzero(case.trait == 2)[0]]
    ptree = orc.prune_for_missing(case.tree, missing + [None])
    ops, tips = orc.tree_program(ptree, index_of)
    assert len(tips) == case.K
    gb = orc.pack_rows(case.genes)
    tb = orc.pack_rows((case.trait == 1)[None].astype(np.uint8))[0]
    mb = orc.pack_rows((case.trait != 2)[None].astype(np.uint8))[0]
    obs = np.zeros((G, 3), dtype=np.int32)
    flags = np.zeros((G, P), dtype=np.uint8)
    for g in range(G):
        obs[g], flags[g] = orc.tree_permute(ops, tips, gb[g], tb, mb, N, EXCEED_TRAIT_INDEX, P,
                                            EXCEED_LABEL_SEED)
    pairs = np.zeros((G, P, 3), dtype=np.int32)
    npos = int((case.trait == 1).sum())
    gstate = np.where(case.genes[:, tips] == 1, 0, 2)
    for p in range(P):
        lab = orc.perm_labels(EXCEED_LABEL_SEED, EXCEED_TRAIT_INDEX, p, mb, npos, N)
        lab01 = np.unpackbits(lab.view(np.uint8), bitorder="little")[:N]
        lstate = np.where(lab01[tips] == 1, 0, 1)
        for g in range(G):
            pairs[g, p] = orc.tree_dp(ops, (gstate[g] + lstate).astype(np.uint8))
    case.ptree, case.obs, case.flags, case.pairs = ptree, obs, flags, pairs
    case.ties = exact_exceed(obs, pairs)[1]
    return case


_exceed_cache = {}


def exceed_references(orc):
    """The five cases with the oracle's results: computed once per process, shared by the host
    test of the conditions below and the device tests; nobody writes to them."""
    if "cases" not in _exceed_cache:
        _exceed_cache["cases"] = [exceed_reference(orc, exceed_case(K, cat)) for K, cat in EXCEED_CASES]
    return _exceed_cache["cases"]


def exceed_conditions(cases):
    """What keeps test A from passing vacuously, over all cases together and from the oracle's
    results alone."""
    flags = np.concatenate([c.flags.ravel() for c in cases])
    obs = np.concatenate([c.obs for c in cases])
    return {
        "a flag is 1": bool((flags == 1).any()),
        "a flag is 0": bool((flags == 0).any()),
        "an exact tie": any(bool(c.ties.any()) for c in cases),
        "a gene on the opposing side": bool((obs[:, 2] > obs[:, 1]).any()),
        "a gene with pro == anti > 0": bool(((obs[:, 1] == obs[:, 2]) & (obs[:, 1] > 0)).any()),
    }


# ---------------------------------------------------------------------------------------------
# B: --collapse hash tables
# ---------------------------------------------------------------------------------------------
HASH_SIZES = (1, 127, 128, 129, 257, 2100)      # one quad, its edges, a quad tail, 17 quads


def hash_case(N):
    """genes (G, N): 20 random rows, then the sweep -- a random base row and base ^ e_i for
    EVERY isolate i (N + 1 rows) --, 20 more random rows, and at the end exact copies of three
    rows: the first random row, the base and a row from the middle of the sweep.  With more
    than 256 genes every copy sits in another 256-gene block than its original.  valid (3, N):
    all valid; a random 10 % missing, always isolates 0 and N - 1; all missing but one isolate."""
    rng = np.random.default_rng(7000 + N)
    base = (rng.random(N) < 0.5).astype(np.uint8)
    sweep = np.vstack([base[None], base[None] ^ np.eye(N, dtype=np.uint8)])
    rand = (rng.random((40, N)) < rng.uniform(0.1, 0.9, (40, 1))).astype(np.uint8)
    copied = np.array([0, 20, 20 + 1 + N // 2])
    genes = np.vstack([rand[:20], sweep, rand[20:]])
    genes = np.ascontiguousarray(np.vstack([genes, genes[copied]]))
    G = genes.shape[0]
    if G > 256:
        assert all(o // 256 != c // 256 for o, c in zip(copied, range(G - 3, G)))
    valid = np.ones((3, N), dtype=np.uint8)
    valid[1, rng.random(N) < 0.1] = 0
    valid[1, [0, N - 1]] = 0
    valid[2] = 0
    valid[2, max(N - 2, 0)] = 1
    return SimpleNamespace(N=N, genes=genes, valid=valid, sweep=slice(20, 20 + N + 1), copied=copied)


# ---------------------------------------------------------------------------------------------
# C: UPGMA past one stride of the device loops (1024 in k_upgma_merge, 256 in k_upgma_rowmin)
# ---------------------------------------------------------------------------------------------
UPGMA_CASES = {1025: (300, None),       # n: (columns, planted structure)
               1300: (40, "dup"),
               1280: (300, "tail")}
UPGMA_TAIL_TRIPLES = ((5, 1100, 1200), (700, 1024, 1279), (1023, 1150, 1151))


def upgma_case(n):
    """(var, names, counts): n isolates x variable columns at density 0.3 and their Hamming
    counts.  1025: few ties, the first n at which every 1024-stride loop takes a second turn.
    1300 "dup": the second half duplicates the first -- hundreds of zero-distance ties between
    rows more than 512 apart and many equal positive distances.
    1280 "tail": the distance matrix is symmetric and the tie order prefers the smaller row, so
    in the two cases above the winning cell of every merge sits in a row below 1024 and the
    second turn of k_upgma_merge's minimum reduction never decides anything.  Here, per triple
    (a, b, c), rows b and c (both past 1024) are identical and one bit away from row a: the
    first merges are the (b, c) at distance 0, found only in the reduction's second turn;
    a reduction that stops at 1024 rows merges (a, b) first, which is another tree."""
    cols, plant = UPGMA_CASES[n]
    rng = np.random.default_rng(9000 + n)
    X = (rng.random((n, cols)) < 0.3).astype(np.uint8)
    if plant == "dup":
        X[n // 2:] = X[:n - n // 2]
    elif plant == "tail":
        for k, (a, b, c) in enumerate(UPGMA_TAIL_TRIPLES):
            X[b] = X[a]
            X[b, k] ^= 1
            X[c] = X[b]
    tot = X.sum(axis=0)
    var = np.ascontiguousarray(X[:, (tot > 0) & (tot < n)])
    Xi = var.astype(np.int64)
    cnt = Xi @ (1 - Xi).T + (1 - Xi) @ Xi.T
    return var, ["s%d" % i for i in range(n)], cnt
