"""Synthetic rejection regions for the permutation kernels, and their numpy reference.

The permutation kernels compute r[t][g] = #{pi : u < lo or u >= hi1}, u = the overlap of the gene's
minority row with the permuted labels, for an acceptance interval [lo, hi1) that is an INPUT of the launch.
Under the interval Fisher derives from the data only two mid-distribution thresholds of u are ever seen;
with intervals chosen by the test -- edges, point intervals [v, v + 1), random ones -- every value of u is
observable through r.  This module builds the gene matrices, traits and interval families of
tests/test_gpu_permute_probe.py and the reference they are compared with: the labels of the CPU oracle's
generator, a float64 matrix product for u (exact: every entry is an integer <= 2048 ... N), a compare.

Plain numpy: neither torch nor the engine is imported here, and the oracle only inside the functions that
are handed it.
"""
import numpy as np

ONE_HOTS = (0, 1, 31, 32, 63, 64, 1023, 1024, 2046, 2047)
SEG_ROWS = 20_352          # isolates per LDS segment of k_permute_seglists


# ------------------------------------------------------------------ problems ------
def probe_traits(N, seed, T=5):
    """Traits 0..2 as the stagger tests build them (two different sets of missing values); with T = 5 also
    a trait with one positive (missing as trait 2) and one with nval - 1 positives (nothing missing)."""
    rng = np.random.default_rng(seed)
    traits = (rng.random((3, N)) < 0.4).astype(np.uint8)
    traits[1, ::29] = 2
    traits[2, 5::17] = 2
    if T == 3:
        return traits
    assert T == 5
    one = np.zeros(N, dtype=np.uint8)
    one[5::17] = 2
    valid = np.flatnonzero(one != 2)
    one[valid[len(valid) // 2]] = 1
    most = np.ones(N, dtype=np.uint8)
    most[int(rng.integers(0, N))] = 0
    return np.vstack([traits, one[None], most[None]])


def one_hot_isolates(N, extra=()):
    return sorted({i for i in ONE_HOTS + tuple(extra) if 0 <= i < N} | {N - 1})


def probe_genes(G, N, traits, seed, extra_hots=(), with_empty=True):
    """(G, N) 0/1 matrix.  The first rows are fixed: an absent and a core gene (with_empty), the one-hot
    genes and their complements, a gene with exactly N / 2 carriers (even N) and one with N // 2 + 1 (the
    flip tie and the first flipped count), a gene carried by exactly the isolates missing in trait 1 (u = 0
    there, whatever the permutation).  The rest is random over the frequencies 0.02 .. 0.98; without
    with_empty a random row that came out empty or full gets one isolate changed, so that every list of the
    matrix has an entry.  Returns (genes, names of the fixed rows)."""
    rng = np.random.default_rng(seed)
    fixed, names = [], []

    def add(row, name):
        fixed.append(np.asarray(row, dtype=np.uint8))
        names.append(name)

    if with_empty:
        add(np.zeros(N), "absent")
        add(np.ones(N), "core")
    hots = one_hot_isolates(N, extra_hots)
    for i in hots:
        row = np.zeros(N, dtype=np.uint8)
        row[i] = 1
        add(row, "hot%d" % i)
    for i in hots:
        row = np.ones(N, dtype=np.uint8)
        row[i] = 0
        add(row, "cold%d" % i)
    perm = rng.permutation(N)
    if N % 2 == 0:
        row = np.zeros(N, dtype=np.uint8)
        row[perm[:N // 2]] = 1
        add(row, "half")
    row = np.zeros(N, dtype=np.uint8)
    row[perm[:N // 2 + 1]] = 1
    add(row, "half+1")
    add(traits[1] == 2, "missing1")
    assert len(fixed) <= G, "G = %d is too small for the %d fixed rows" % (G, len(fixed))
    genes = (rng.random((G, N)) < rng.uniform(0.02, 0.98, (G, 1))).astype(np.uint8)
    if not with_empty:
        n1 = genes.sum(1)
        for g in np.flatnonzero((n1 == 0) | (n1 == N)):
            genes[g, g % N] ^= 1
    genes[:len(fixed)] = np.array(fixed)
    return genes, names


def identity_genes(N):
    """The N x N identity and its complement, G = 2 N: every isolate column is read once by a list of one."""
    eye = np.eye(N, dtype=np.uint8)
    return np.vstack([eye, 1 - eye])


# ------------------------------------------------------------------ reference ------
def flip_rule(genes):
    """flipped[g]: the list holds the isolates WITHOUT the gene -- more than half carry it."""
    genes = np.asarray(genes)
    return 2 * genes.sum(1, dtype=np.int64) > genes.shape[1]


def minority_rows(genes, flipped):
    return (np.asarray(genes, dtype=np.uint8) ^ np.asarray(flipped, dtype=np.uint8)[:, None]).astype(np.uint8)


def host_order(L):
    """A slot order for tests that have no device: stable sort by descending list length."""
    return np.argsort(-np.asarray(L, dtype=np.int64), kind="stable")


def check_order(order, L):
    """order is a permutation of the genes, sorted by descending list length."""
    order = np.asarray(order, dtype=np.int64)
    assert np.array_equal(np.sort(order), np.arange(len(L))), "order is not a permutation"
    assert np.all(np.diff(np.asarray(L)[order]) <= 0), "slots are not sorted by descending list length"


def pack_bits(dense01):
    """(R, N) 0/1 -> (R, W64) uint64, bit i of word w = column 64 w + i (the oracle's row form)."""
    dense01 = np.ascontiguousarray(dense01, dtype=np.uint8)
    R, N = dense01.shape
    W = (N + 63) // 64
    by = np.packbits(dense01, axis=1, bitorder="little")
    out = np.zeros((R, W * 8), dtype=np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u8")


def trait_bits(traits):
    return pack_bits(traits == 1), pack_bits(traits != 2)


def oracle_labels(orc, seed, traits, P, perm_base=0):
    """lab[t][pi][i] in {0, 1}: the oracle's labels of permutations perm_base .. perm_base + P - 1 (a
    multiple of 32), unpacked as tests/test_gpu_parity.py::test_perm_labels_bit_exact does."""
    assert perm_base % 32 == 0
    T, N = traits.shape
    _tb, mb = trait_bits(traits)
    lab = np.zeros((T, P, N), dtype=np.uint8)
    for t in range(T):
        npos = int((traits[t] == 1).sum())
        for b in range(-(-P // 32)):
            blk = orc.perm_block(seed, t, perm_base // 32 + b, mb[t], npos, N)
            bits = np.unpackbits(blk.view(np.uint8), axis=1, bitorder="little")[:, :N]
            n = min(32, P - 32 * b)
            lab[t, 32 * b:32 * b + n] = bits[:n]
    return lab


def overlap_counts(minority, lab):
    """u[t][g][pi] = sum_i minority[g][i] lab[t][pi][i], by a float64 matrix product (exact)."""
    m = np.asarray(minority, dtype=np.float64)
    u = np.stack([m @ lab[t].T.astype(np.float64) for t in range(lab.shape[0])])
    ui = np.rint(u).astype(np.int64)
    assert np.array_equal(ui, u)
    return ui


def slot_limits(L, npos, order):
    """m[t][k] = min(L of slot k, npos of trait t): the largest u there can be."""
    return np.minimum(np.asarray(L, dtype=np.int64)[np.asarray(order)][None, :],
                      np.asarray(npos, dtype=np.int64)[:, None])


def check_regions(lo, hi1, m):
    """The domain every interval of the probes lies in: 0 <= lo <= hi1 <= m + 1."""
    lo, hi1 = np.asarray(lo, dtype=np.int64), np.asarray(hi1, dtype=np.int64)
    assert lo.shape == hi1.shape == m.shape
    assert np.all(0 <= lo) and np.all(lo <= hi1) and np.all(hi1 <= m + 1), "interval outside 0 <= lo <= hi1 <= m + 1"
    return lo, hi1


def r_ref(u, order, lo, hi1):
    """r[t][order[k]] = #{pi : u < lo[t][k] or u >= hi1[t][k]} for slot-order intervals; (T, G) uint32."""
    order = np.asarray(order, dtype=np.int64)
    us = u[:, order, :]
    cnt = ((us < np.asarray(lo)[..., None]) | (us >= np.asarray(hi1)[..., None])).sum(-1)
    r = np.empty(cnt.shape, dtype=np.uint32)
    r[:, order] = cnt
    return r


def gene_order_crit(lo, hi1, order, flipped, npos):
    """Slot-order [lo, hi1) of u -> gene-order (base, span) of the dense kernel's a (accept a in
    [base, base + span); span 0: every permutation counts) -- the inverse of k_lists_crit.  int32 (T, G, 2)."""
    lo, hi1 = np.asarray(lo, dtype=np.int64), np.asarray(hi1, dtype=np.int64)
    order = np.asarray(order, dtype=np.int64)
    fl = np.asarray(flipped, dtype=bool)[order][None, :]
    npos = np.asarray(npos, dtype=np.int64)[:, None]
    span = hi1 - lo
    base = np.where(span == 0, 0, np.where(fl, npos - hi1 + 1, lo))
    assert np.all(base >= 0)
    crit = np.empty(lo.shape + (2,), dtype=np.int32)
    crit[:, order, 0] = base
    crit[:, order, 1] = span
    return crit


def slot_regions_from_crit(crit, order, flipped, npos):
    """Gene-order (base, span) -> slot-order (lo, hi1): k_lists_crit, restated."""
    order = np.asarray(order, dtype=np.int64)
    c = np.asarray(crit, dtype=np.int64)[:, order, :]
    fl = np.asarray(flipped, dtype=bool)[order][None, :]
    npos = np.asarray(npos, dtype=np.int64)[:, None]
    base, span = c[..., 0], c[..., 1]
    lo = np.where(fl, npos - base - span + 1, base)
    hi1 = np.where(fl, npos - base + 1, base + span)
    return np.where(span == 0, 0, lo), np.where(span == 0, 0, hi1)


# ------------------------------------------------------------------ region families ------
def edge_regions(m):
    """name -> (lo, hi1), each shaped like m."""
    z = np.zeros_like(m)
    return {
        "(0,0)": (z, z),                  # r == P
        "[0,m+1)": (z, m + 1),            # r == 0
        "[0,1)": (z, z + 1),
        "[m,m+1)": (m, m + 1),
        "[1,m+1)": (z + 1, m + 1),
        "[0,m)": (z, m),
    }


def random_regions(m, seed):
    """(lo, hi1) independent per (trait, slot), uniform on the pairs 0 <= lo <= hi1 <= m + 1: pairs with
    repetition from m + 2 values = two distinct values a < b of m + 3, (lo, hi1) = (a, b - 1)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, m + 3)
    b = rng.integers(0, m + 2)
    b = b + (b >= a)
    lo, hi = np.minimum(a, b), np.maximum(a, b) - 1
    return check_regions(lo, hi, m)


def sweep_launches(u, order, m):
    """The point intervals [v, v + 1) of the sweep: launch j has v = clamp(umin - 1 + j, 0, m) per
    (trait, slot), j < J = max(umax - umin) + 3 -- every value u takes, and one on either side."""
    us = u[:, np.asarray(order, dtype=np.int64), :]
    umin, umax = us.min(-1), us.max(-1)
    J = int((umax - umin).max()) + 3
    return [np.clip(umin - 1 + j, 0, m) for j in range(J)]


# ------------------------------------------------------------------ the oracle's own regions ------
P_TIE = 1.0 + 1e-9


def oracle_crit(orc, genes, traits):
    """Gene-order (base, span) from the oracle's acceptance rule.  orc_permute_r counts a permutation when
    its table is as or less probable than the observed one, w(a) <= w(a_obs) (1 + 1e-14), which is
    "p(a) <= p(a_obs)" for the two-sided p of orc_fisher: p is the sum of the weights <= w (1 + 1e-14), so
    a table inside the region sums a subset of the observed table's terms (p(a) <= p(a_obs) up to the last
    bits), and one outside sums at least one more term that is larger than every term of p(a_obs), hence
    p(a) >= p(a_obs) (1 + 1 / len), len <= N / 2 + 1 the size of the support.  P_TIE sits between the two.
    Here that rule is applied through fisher_many to the table of every a of the support."""
    genes = np.asarray(genes, dtype=np.int64)
    T, N = traits.shape
    G = genes.shape[0]
    crit = np.zeros((T, G, 2), dtype=np.int32)
    for t in range(T):
        pos, valid = (traits[t] == 1).astype(np.int64), (traits[t] != 2).astype(np.int64)
        npos, nval = int(pos.sum()), int(valid.sum())
        nneg = nval - npos
        mg, aobs = genes @ valid, genes @ pos
        tables, spans = [], []
        for g in range(G):
            if npos == 0 or nneg == 0 or mg[g] == 0 or mg[g] == nval:
                spans.append(None)                                 # skipped: every permutation counts
                continue
            a = np.arange(max(0, mg[g] + npos - nval), min(mg[g], npos) + 1)
            tables.append(np.stack([a, npos - a, mg[g] - a, nneg - mg[g] + a], axis=1))
            spans.append((int(a[0]), len(a)))
        if not tables:
            continue
        _odds, p = orc.fisher_many(np.concatenate(tables))
        at = 0
        for g in range(G):
            if spans[g] is None:
                continue
            a0, n = spans[g]
            pg = p[at:at + n]
            at += n
            accept = np.flatnonzero(~(pg <= pg[aobs[g] - a0] * P_TIE))
            if len(accept):
                assert accept[-1] - accept[0] + 1 == len(accept), "the acceptance set is not an interval"
                crit[t, g] = (a0 + accept[0], len(accept))
    return crit
