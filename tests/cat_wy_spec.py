"""Spec S22 in plain Python and numpy: Westfall-Young single-step maxT over the statistics of
the categorical traits.  A helper, not a test; written from the specification, independently of the kernels and of the
engine, on top of categorical_spec (S20) and gcmh_spec (S21), whose tables, statistics and permuted rows it takes as
they are.  Doubles throughout: Python floats and numpy float64 multiply, add and divide as IEEE binary64, one rounding
per operation, which is what the spec fixes."""
from fractions import Fraction

import numpy as np

import categorical_spec as cs
import gcmh_spec as gs

BAND = 1e-9                                             # S3's band
ONE_MINUS_BAND = 1.0 - BAND
MAX_C = 16320 * 16320                                   # |c_k| <= 16320^2 < 2^29: exact in int32 and in a double


def inv_of(nk):
    """inv[k] = 1.0 / (double)n_k where n_k > 0, else 0.0."""
    return [1.0 / float(x) if x > 0 else 0.0 for x in nk]


def ivm_of(a, nk):
    """1.0 / ((double)m (double)(n - m)) where the gene is testable by S20's rule, else 0.0."""
    n, m = sum(nk), sum(a)
    return 1.0 / (float(m) * float(n - m)) if cs.testable(a, nk) else 0.0


def stat(a, nk, ivm):
    """s of a cell: the table a of a gene (observed or permuted: m = sum a either way) against the class sizes nk."""
    n, m = sum(nk), sum(a)
    inv = inv_of(nk)
    tot = 0.0
    for ak, n_k, iv in zip(a, nk, inv):                 # ascending k, classes with n_k > 0
        if n_k > 0:
            c = n * ak - m * n_k                        # exact
            assert abs(c) <= MAX_C
            e = float(c) * float(c)
            tot = tot + e * iv
    return tot * ivm


def stats(a, nk, ivm):
    """stat() over arrays: a int [.., G, K], nk K ints, ivm float64 [G] -> float64 [.., G]."""
    a = np.asarray(a, dtype=np.int64)
    n, m = int(sum(nk)), a.sum(axis=-1)
    inv = inv_of(nk)
    tot = np.zeros(a.shape[:-1])
    for k, n_k in enumerate(nk):
        if n_k > 0:
            c = n * a[..., k] - m * int(n_k)
            assert np.abs(c).max(initial=0) <= MAX_C
            cf = c.astype(np.float64)
            tot = tot + (cf * cf) * inv[k]
    return tot * np.asarray(ivm, dtype=np.float64)


def thr_of(s_obs):
    """The comparison point of the chi-square maximum: one multiplication."""
    return s_obs * ONE_MINUS_BAND


def maxs(S):
    """S float64 [P, G] (the statistic of every gene under every permuted row) -> float64 [P], the maximum over genes."""
    return np.asarray(S, dtype=np.float64).max(axis=1)


def r_fwer(mx, thr):
    """#{pi : maxs[pi] >= thr[g]} per gene, doubles compared exactly."""
    mx, thr = np.asarray(mx, dtype=np.float64), np.asarray(thr, dtype=np.float64)
    return (mx[None, :] >= thr[:, None]).sum(axis=1)


def chi2_problem(genes, codes, K=cs.MAX_CLASSES):
    """One trait of S20: genes [G][N] of 0/1, codes N ints -> dict(nk, inv, a [G][K], ivm, s_obs, thr [G])."""
    nk = cs.sizes(codes, K)
    a = [cs.table(list(g), codes, K) for g in genes]
    ivm = [ivm_of(x, nk) for x in a]
    s_obs = [stat(x, nk, v) for x, v in zip(a, ivm)]
    return dict(nk=nk, inv=inv_of(nk), a=a, ivm=ivm, s_obs=s_obs, thr=[thr_of(s) for s in s_obs])


def chi2_cells(genes, rows, pr, K=cs.MAX_CLASSES):
    """s of every (row, gene): float64 [P, G]."""
    return np.array([[stat(cs.table(list(g), row, K), pr["nk"], v) for g, v in zip(genes, pr["ivm"])] for row in rows],
                    dtype=np.float64).reshape(len(rows), len(genes))


def inside_band(a_perm, a_obs, nk):
    """A permuted table strictly below the observed X2 and within twice the band of it, in the rationals: where no
    table is, a gene's own family-wise count equals its exceedance count."""
    if not cs.testable(a_obs, nk):
        return False
    obs, perm = cs.x2_exact(a_obs, nk), cs.x2_exact(a_perm, nk)
    return obs * (1 - Fraction(2, 10 ** 9)) <= perm < obs


def gcmh_problem(genes, codes, strata, S):
    """One trait of S21: -> dict(nsk, st [G] (gcmh_spec.statistic's dicts), s_obs = q, thr [G])."""
    nsk = gs.margins(codes, strata, S)
    st = [gs.statistic(*gs.counts(list(g), codes, strata, S), nsk) for g in genes]
    return dict(nsk=nsk, st=st, s_obs=[x["q"] for x in st], thr=[x["thr"] for x in st])


def gcmh_cells(genes, rows, pr, strata, S):
    """Q of every (row, gene) under the gene's form: float64 [P, G]."""
    return np.array([[gs.q_of(gs.counts(list(g), row, strata, S)[0], x["form"]) for g, x in zip(genes, pr["st"])]
                     for row in rows], dtype=np.float64).reshape(len(rows), len(genes))
