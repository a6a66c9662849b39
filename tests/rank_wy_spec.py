"""Spec S17 in plain Python and numpy: Westfall-Young single-step maxT over the rank statistics
of the quantitative traits.  A helper, not a test; written from the specification, independently of the kernels and
of the engine, on top of ranksum_spec (S15) and vanelteren_spec (S16), whose ranks, statistics and permuted rows it
takes as they are.  Doubles throughout: Python floats and numpy float64 multiply and divide as IEEE binary64, one
rounding per operation, which is what the spec fixes."""
import math

import numpy as np

import ranksum_spec as rsp
import vanelteren_spec as vsp

CC_RANKSUM = 1                                          # S15: z = (|D| - 1) / (2 sqrt var)
CC_VANELTEREN = 0                                       # S16: no continuity correction
MAX_E = 16320 * 16319                                   # 266 326 080 < 2^28: the largest |D| the rank kernels carry


def var_ranksum(m, n, tiesum):
    """S15's variance of a gene over m of the n valid isolates, operations in S15's order; 0.0 where untestable."""
    if n < 2 or m == 0 or m == n:
        return 0.0
    f = float(n + 1) - float(tiesum) / (float(n) * float(n - 1))
    if f <= 0:
        return 0.0
    return (float(m) * float(n - m) / 12.0) * f


def var_vanelteren(ms, pl):
    """S16's variance of a gene with per-stratum counts ms under the plan pl (vanelteren_spec.tail's)."""
    var = vsp.tail(0, ms, pl)[1]
    return var if var > 0.0 else 0.0


def inverse(var):
    return 1.0 / var if var > 0.0 else 0.0


def stat(D, cc, iv):
    """s of a cell: E = max(0, |D| - cc), two multiplications, each rounded on its own."""
    e = float(max(0, abs(int(D)) - cc))
    return (e * e) * iv


def stats(D, cc, iv):
    """stat() over arrays: D int [G, ...], iv float64 [G] -> float64 of D's shape."""
    D = np.asarray(D, dtype=np.int64)
    assert np.abs(D).max(initial=0) <= MAX_E
    e = np.maximum(0, np.abs(D) - cc).astype(np.float64)
    iv = np.asarray(iv, dtype=np.float64).reshape((-1,) + (1,) * (D.ndim - 1))
    return (e * e) * iv


def p_of(s):
    """The asymptotic two-sided p that s stands for: s = 4 z^2."""
    return math.erfc(math.sqrt(s / 4.0) / math.sqrt(2.0))


def maxs(D, cc, iv):
    """D int [G, P] (the statistic of every gene under every permuted row) -> float64 [P], the maximum over genes."""
    return stats(D, cc, iv).max(axis=0)


def r_fwer(mx, s_obs):
    """#{pi : maxs[pi] >= s_obs[g]} per gene, doubles compared exactly."""
    mx, s_obs = np.asarray(mx, dtype=np.float64), np.asarray(s_obs, dtype=np.float64)
    return (mx[None, :] >= s_obs[:, None]).sum(axis=1)


def r_count(D, d_obs):
    """S15's / S16's exceedance count #{pi : |D[g][pi]| >= |d_obs[g]|}."""
    D, d_obs = np.asarray(D, dtype=np.int64), np.asarray(d_obs, dtype=np.int64)
    return (np.abs(D) >= np.abs(d_obs)[:, None]).sum(axis=1)


def ranksum_problem(genes, values):
    """One trait of S15: genes [G][N] of 0/1, values N floats (nan = missing) -> dict(valid, rc, n, tiesum, d [G],
    m [G], var [G], iv [G], s_obs [G])."""
    valid, rc, n, tiesum, _ = rsp.ranks(list(values))
    dm = [rsp.statistic(list(g), valid, rc) for g in genes]
    var = [var_ranksum(m, n, tiesum) for _d, m in dm]
    iv = [inverse(v) for v in var]
    return dict(valid=valid, rc=rc, n=n, tiesum=tiesum, d=[d for d, _m in dm], m=[m for _d, m in dm], var=var, iv=iv,
                s_obs=[stat(d, CC_RANKSUM, x) for (d, _m), x in zip(dm, iv)], cc=CC_RANKSUM)


def vanelteren_problem(genes, values, strata, S):
    """One trait of S16: -> dict(pl, d [G], ms [G][S], var [G], iv [G], s_obs [G])."""
    pl = vsp.plan(list(values), list(strata), S)
    dm = [vsp.statistic(list(g), pl) for g in genes]
    var = [var_vanelteren(ms, pl) for _d, ms in dm]
    iv = [inverse(v) for v in var]
    return dict(pl=pl, d=[d for d, _ms in dm], ms=[ms for _d, ms in dm], var=var, iv=iv,
                s_obs=[stat(d, CC_VANELTEREN, x) for (d, _ms), x in zip(dm, iv)], cc=CC_VANELTEREN)


def permuted(genes, rows):
    """genes [G][N] of 0/1, rows [P][N] of ints -> D int64 [G, P]."""
    return np.asarray(genes, dtype=np.int64) @ np.asarray(rows, dtype=np.int64).reshape(len(rows), -1).T
