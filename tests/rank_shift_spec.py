"""Spec S19 of DESIGN.md in plain numpy: the Hodges-Lehmann shift of the rank-sum test and its confidence limits.

Two statements of the same order statistics: brute force (sort the K differences) and the bisection over the
order-preserving keys of the doubles that the kernel uses, with the count taken by brute force.  Nothing here knows
how the kernel counts."""
import math
import statistics
import struct

import numpy as np

MAX_ABS = 1e150


def zq_of(level):
    return statistics.NormalDist().inv_cdf(0.5 + float(level) / 2.0)


def s15_var(x, m):
    """S15's variance of a gene with m carriers among the valid values x, operations in its order; 0.0 where the gene
    is untestable."""
    n = int(x.size)
    if n < 2 or m <= 0 or m >= n:
        return 0.0
    tau = np.unique(x, return_counts=True)[1].astype(np.int64)
    tiesum = int(np.sum(tau ** 3 - tau))
    f = float(n + 1) - float(tiesum) / (float(n) * float(n - 1))
    if not f > 0.0:
        return 0.0
    mm = float(m) * float(n - m)
    return (mm / 12.0) * f


def ca_unfloored(K, zq, var):
    return 0.5 * float(K) - zq * math.sqrt(var)


def differences(a, b):
    """The K differences fl(a_i - b_j), ascending."""
    return np.sort(np.subtract.outer(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)).ravel())


def order_statistic(d_sorted, rank):
    """d_(rank), rank 1-based, a zero as +0.0."""
    return float(d_sorted[rank - 1]) + 0.0


def split(values, bits):
    """(carriers' values, non-carriers' values, all valid values) of a trait row (nan = missing; -0.0 taken as +0.0)
    and a gene's 0/1 row."""
    values = np.asarray(values, dtype=np.float64)
    valid = ~np.isnan(values)
    if np.any(np.abs(values[valid]) > MAX_ABS):
        raise ValueError("a value above 1e150 in magnitude")
    bits = np.asarray(bits).astype(bool)
    return values[valid & bits] + 0.0, values[valid & ~bits] + 0.0, values[valid] + 0.0


def shift_from(d, K, ca):
    """(shift, lower, upper) from the order statistics d(rank) of K differences at the given ca."""
    lo, hi = d((K - 1) // 2 + 1), d(K // 2 + 1)
    shift = (lo + hi) * 0.5 + 0.0
    if ca >= 1:
        return shift, d(ca), d(K + 1 - ca)
    return shift, -math.inf, math.inf


def shift_spec(values, bits, level=0.95, ca=None, partition=False):
    """(shift, lower, upper, ca, unfloored ca) of one (trait, gene).  ``ca``: use this one instead of the spec's (the
    limits at a device's own ca).  ``partition``: select with numpy.partition instead of a full sort (large K)."""
    a, b, x = split(values, bits)
    var = s15_var(x, a.size)
    if var == 0.0:
        return 0.0, -math.inf, math.inf, 0, 0.0
    K = a.size * b.size
    raw = ca_unfloored(K, zq_of(level), var)
    if ca is None:
        ca = min(int(math.floor(raw)), K // 2)
    diffs = np.subtract.outer(a, b).ravel()
    if partition:
        ranks = {(K - 1) // 2 + 1, K // 2 + 1} | ({ca, K + 1 - ca} if ca >= 1 else set())
        diffs = np.partition(diffs, [r - 1 for r in sorted(ranks)])
    else:
        diffs.sort()
    return shift_from(lambda r: order_statistic(diffs, r), K, ca) + (ca, raw)


# ---- the key bisection, stated on its own ------------------------------------------------------------------------
def key_of(v):
    """Order-preserving 64-bit key of a double: every bit of a negative flipped, the top bit of a non-negative set."""
    b = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b | (1 << 63))


def value_of(k):
    b = (k & 0x7FFFFFFFFFFFFFFF) if k >> 63 else (~k & 0xFFFFFFFFFFFFFFFF)
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def select_by_bisection(a, b, rank):
    """d_(rank) of the differences fl(a_i - b_j) as the smallest key whose value has at least ``rank`` differences at
    or below it: at most 64 halvings of the key range between the smallest and the largest possible difference."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    diffs = np.subtract.outer(a, b)
    x = np.concatenate([a, b])
    lo, hi = key_of(float(x.min() - x.max())), key_of(float(x.max() - x.min()))
    steps = 0
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if int(np.count_nonzero(diffs <= value_of(mid))) >= rank:
            hi = mid
        else:
            lo = mid + 1
        steps += 1
    assert steps <= 64
    return value_of(hi) + 0.0
