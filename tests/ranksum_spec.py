"""Spec S15 in plain Python: the rank-sum test of a measured value against gene presence and
its value permutations.  A helper, not a test; written from the specification, independently of the kernels and of
the engine's host ranking, on top of the oracle's Philox block function only (the shape of strata_spec.py).  The
bfrag_* functions restate the byte order of scoary_permute_ranksum's B operand from the words of the public header."""
import bisect
import math

import numpy as np

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


def chunks(N):
    """Chunks of 256 isolates that cover N: the B operand's K is padded to that many."""
    return -(-N // 256)


def bfrag_bytes(N, P, T):
    """Bytes of the B operand of T traits x P permutations: a chunk of a stage of 64 permutations is 32 KB."""
    return T * -(-P // 64) * chunks(N) * 32768


def bfrag_pack(dig):
    """dig: int8 [T][64 S][256 chunks][2] -- the (hi, lo) digits of every (trait, column, isolate) of whole stages
    and whole chunks -> the bytes, in the order include/scoary_hip.h states:
    [t][stage of 64][K-step of 32 isolates][plane hi, lo][column tile of 32][lane of 64] x 16 bytes, lane l of a
    fragment = column 64 stage + 32 tile + (l & 31), isolates 32 K-step + 16 (l >> 5) .. + 15, one per byte."""
    dig = np.asarray(dig, dtype=np.int8)
    T, C, K, _ = dig.shape
    assert C % 64 == 0 and K % 256 == 0
    x = dig.reshape(T, C // 64, 2, 32, K // 32, 2, 16, 2)        # t, stage, tile, l & 31, K-step, l >> 5, byte, plane
    x = x.transpose(0, 1, 4, 7, 2, 5, 3, 6)                      # t, stage, K-step, plane, tile, l >> 5, l & 31, byte
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def bfrag_unpack(buf, T, P, N):
    """The inverse of bfrag_pack: the bytes of a B operand of (T, P, N) -> int8 [T][64 S][256 chunks][2]."""
    S, W = -(-P // 64), 8 * chunks(N)
    buf = np.asarray(buf).reshape(-1).view(np.int8)
    assert buf.size == bfrag_bytes(N, P, T), (buf.size, bfrag_bytes(N, P, T))
    x = buf.reshape(T, S, W, 2, 2, 2, 32, 16).transpose(0, 1, 4, 6, 2, 5, 7, 3)
    return np.ascontiguousarray(x).reshape(T, 64 * S, 32 * W, 2)


def bfrag_encode(rows, N):
    """rows[T][P][N] of ints, |Rc| <= 16 319 -> the bytes of the B operand: permutation p in column p, the columns
    from P to the end of the last stage and the isolates from N to the end of the last chunk zero."""
    rows = np.asarray(rows, dtype=np.int64)
    T, P, n = rows.shape
    assert n == N and np.abs(rows).max(initial=0) < MAX_ISOLATES
    lo = (rows + 64) % 128 - 64                                   # digits(), on arrays
    dig = np.zeros((T, 64 * -(-P // 64), 256 * chunks(N), 2), dtype=np.int8)
    dig[:, :P, :N, 0] = (rows - lo) // 128
    dig[:, :P, :N, 1] = lo
    return bfrag_pack(dig)


def bfrag_decode(buf, T, P, N):
    """-> (rows int64 [T][P][N] = 128 hi + lo, digits int8 [T][P][N][2], the K pad int8 [T][P][256 chunks - N][2],
    the columns at and past P int8 [T][64 S - P][256 chunks][2])."""
    dig = bfrag_unpack(buf, T, P, N)
    d = dig[:, :P, :N].astype(np.int64)
    return 128 * d[..., 0] + d[..., 1], dig[:, :P, :N], dig[:, :P, N:], dig[:, P:]


def r_q(genes, rows, d_obs):
    """genes: G 0/1 rows; rows: the permuted rows of the batch; d_obs [G] -> [G] exceedance counts."""
    out = []
    for gene, d in zip(genes, d_obs):
        on = [i for i, g in enumerate(gene) if g]
        out.append(sum(1 for row in rows if abs(sum(row[i] for i in on)) >= abs(d)))
    return out
