"""Spec S15 in plain Python: the rank-sum test of a measured value against gene presence and
its value permutations.  A helper, not a test; written from the specification, independently of the kernels and of
the engine's host ranking, on top of the oracle's Philox block function only (the shape of strata_spec.py)."""
import bisect
import math

from oracle import oracle as orc

DOM_RANK = 0x53434F51                                   # "SCOQ"
MAX_ISOLATES = 16320


def ranks(values):
    """values: N floats, nan = missing -> (valid [N] of 0/1, rc [N] of ints, n, tiesum, tie groups)."""
    valid = [0 if math.isnan(x) else 1 for x in values]
    xs = [x for x in values if not math.isnan(x)]
    n = len(xs)
    srt = sorted(xs)
    rc = []
    for x in values:
        if math.isnan(x):
            rc.append(0)
            continue
        less = bisect.bisect_left(srt, x)                # #{j: x_j < x}
        equal = bisect.bisect_right(srt, x) - less       # #{j: x_j = x}
        rc.append(2 * less + equal + 1 - (n + 1))
    counts = {}
    for x in xs:
        counts[x] = counts.get(x, 0) + 1
    tiesum = sum(c ** 3 - c for c in counts.values())
    return valid, rc, n, tiesum, sum(1 for c in counts.values() if c > 1)


def tail(D, m, n, tiesum):
    """(testable, auc, p) of a gene with statistic D over m of the n valid isolates: the S15 expression order."""
    if n < 2 or m == 0 or m == n:
        return False, 0.5, 1.0
    f = float(n + 1) - float(tiesum) / (float(n) * float(n - 1))
    if f <= 0:
        return False, 0.5, 1.0
    var = (float(m) * float(n - m) / 12.0) * f
    z = max(0.0, abs(D) * 0.5 - 0.5) / math.sqrt(var)
    return True, 0.5 + D / (2 * m * (n - m)), math.erfc(z / math.sqrt(2.0))


def statistic(gene, valid, rc):
    """(D, m) of one 0/1 gene row."""
    return (sum(r for g, r in zip(gene, rc) if g), sum(1 for g, v in zip(gene, valid) if g and v))


def perm_row(seed, t, pi, valid, rc):
    """The permuted centred ranks of permutation ``pi`` of trait ``t``: N ints, 0 where invalid."""
    key = [seed & 0xffffffff, seed >> 32]
    members = [i for i, v in enumerate(valid) if v]
    L = [rc[i] for i in members]
    comp = []
    for v, i in enumerate(members):
        w = orc.philox4x32_10([i, pi, t, DOM_RANK], key)
        key64 = int(w[0]) | (int(w[1]) << 32)
        comp.append((key64 & ~0x3FFF) | v)
    assert len(set(comp)) == len(comp)
    order = sorted(range(len(comp)), key=comp.__getitem__)      # order[rho] = the valid index with rank rho
    out = [0] * len(valid)
    for rho, v in enumerate(order):
        out[members[v]] = L[rho]
    return out


def digits(rc):
    """Rc = 128 hi + lo with lo in [-64, 63]."""
    lo = ((rc + 64) % 128) - 64
    return (rc - lo) // 128, lo


def r_q(genes, rows, d_obs):
    """genes: G 0/1 rows; rows: the permuted rows of the batch; d_obs [G] -> [G] exceedance counts."""
    out = []
    for gene, d in zip(genes, d_obs):
        on = [i for i, g in enumerate(gene) if g]
        out.append(sum(1 for row in rows if abs(sum(row[i] for i in on)) >= abs(d)))
    return out
