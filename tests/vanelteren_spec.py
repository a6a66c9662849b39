"""Spec S16 in plain Python: the van Elteren (stratified rank-sum) test of a measured value
against gene presence and its value permutations within strata.  A helper, not a test; written from the
specification, independently of the kernels and of the engine's host ranking, on top of the oracle's Philox block
function and of ranksum_spec's restatement of S15's ranks (S16 defines its ranks as S15's inside a stratum)."""
import math

from oracle import oracle as orc

import ranksum_spec as rsp

MAX_SCORE = 16319
MAX_STRATA = 1024


def strata_bits(S):
    return 0 if S == 1 else (S - 1).bit_length()


def weight(n):
    return 0 if n == 0 else max(1, MAX_SCORE // (n + 1))


def plan(values, strata, S):
    """values: N floats, nan = missing; strata: N ints in [0, S) -> dict of valid [N], score [N], L (the scores of
    the valid isolates by (stratum, isolate)), w [S], n [S], tiesum [S], c [S]."""
    N = len(values)
    valid = [0 if math.isnan(x) else 1 for x in values]
    score, L, w, n, tiesum, c = [0] * N, [], [], [], [], []
    for s in range(S):
        who = [i for i in range(N) if strata[i] == s and valid[i]]
        _valid, rc, ns, ts, _groups = rsp.ranks([values[i] for i in who])
        ws = weight(ns)
        for i, r in zip(who, rc):
            score[i] = ws * r
            L.append(ws * r)
        f = float(ns + 1) - float(ts) / (float(ns) * float(ns - 1)) if ns >= 2 else 0.0
        w.append(ws), n.append(ns), tiesum.append(ts), c.append(float(ws * ws) * f / 12.0)
    return dict(valid=valid, score=score, L=L, w=w, n=n, tiesum=tiesum, c=c, strata=list(strata), S=S)


def statistic(gene, pl, row=None):
    """(D, m_s [S]) of one 0/1 gene row against the plan's scores, or against the permuted row ``row``."""
    a = pl["score"] if row is None else row
    ms = [0] * pl["S"]
    for i, g in enumerate(gene):
        if g and pl["valid"][i]:
            ms[pl["strata"][i]] += 1
    return sum(int(x) for g, x in zip(gene, a) if g), ms


def tail(D, ms, pl):
    """(testable, var, den, auc, p) of a gene with statistic D and per-stratum counts ms: the S16 expression order."""
    var, den = 0.0, 0
    for s in range(pl["S"]):
        var += pl["c"][s] * (float(ms[s]) * float(pl["n"][s] - ms[s]))
        den += pl["w"][s] * ms[s] * (pl["n"][s] - ms[s])
    if not var > 0.0:
        return False, var, den, 0.5, 1.0
    z = (abs(D) * 0.5) / math.sqrt(var)
    return True, var, den, 0.5 + float(D) / (2.0 * float(den)), math.erfc(z / math.sqrt(2.0))


def perm_row(seed, t, pi, pl):
    """The permuted scores of permutation ``pi`` of trait ``t``: N ints, 0 where invalid."""
    key = [seed & 0xffffffff, seed >> 32]
    b = strata_bits(pl["S"])
    members = [i for i, v in enumerate(pl["valid"]) if v]
    comp = []
    for i in members:
        w = orc.philox4x32_10([i, pi, t, rsp.DOM_RANK], key)
        key64 = int(w[0]) | (int(w[1]) << 32)
        comp.append(((pl["strata"][i] << (64 - b)) if b else 0) | (((key64 >> 14) >> b) << 14) | i)
    order = sorted(range(len(comp)), key=comp.__getitem__)      # order[rho] = the valid isolate with rank rho
    out = [0] * len(pl["valid"])
    for rho, v in enumerate(order):
        out[members[v]] = pl["L"][rho]
    return out


def r_counts(genes, rows, d_obs):
    """genes: G 0/1 rows; rows: the permuted rows of the batch; d_obs [G] -> [G] exceedance counts."""
    return rsp.r_q(genes, rows, d_obs)
