"""Spec S11 in plain Python floats and numpy: the Westfall-Young family-wise p of the
Cochran-Mantel-Haenszel statistic -- the support of the pooled count under within-stratum shuffles, the snap of E2,
the table entry u(x) = 1 / (1 + stat(x)), the observed value as the gene's own entry, the single-step counts and the
step-down of S8 over u.  Written from the specification and independently of the kernels; the S10 side (the
accumulation of A, E2 and V) is cmh_spec.py's.  A helper, not a test."""
from fractions import Fraction

import numpy as np

import cmh_spec as S10

TAU = S10.TAU
support = S10.support            # step 1: [lo, hi] = the sum of the strata's hypergeometric supports


def snap(e2):
    """Step 2: E2 rounded to the nearest integer (ties to even, rint) when it lies within tau of it."""
    near = float(np.rint(e2))
    return near if abs(e2 - near) <= TAU else e2


def u_entry(x, e2, var):
    """Step 3: the table entry at the pooled count x, every operation a double rounded on its own."""
    if var == 0.0:
        return 1.0
    delta = abs(float(x) - 0.5 * snap(e2))
    y = min(0.5, delta)
    stat = ((delta - y) * (delta - y)) / var
    return 1.0 / (1.0 + stat)


def u_row(lo, hi, e2, var):
    """u_entry at every count of [lo, hi] as one float64 array: the same operations, element by element (numpy
    rounds every operation of a float64 array on its own; test_cmh_wy_spec.py holds the two to each other)."""
    if var == 0.0:
        return np.ones(hi - lo + 1)
    delta = np.abs(np.arange(lo, hi + 1).astype(np.float64) - 0.5 * snap(e2))
    y = np.minimum(0.5, delta)
    stat = ((delta - y) * (delta - y)) / var
    return 1.0 / (1.0 + stat)


def table(tables):
    """(lo, float64 array u(lo) ... u(hi), A) of one (trait, gene) from its per-stratum (a, m, k, n)."""
    r = S10.cmh(tables)
    lo, hi = support(tables)
    return lo, u_row(lo, hi, r["e2"], r["var"]), r["a"]


def exact_cc_extreme(tables, x):
    """The continuity-corrected rule in Fractions: the count x is as or more extreme than the observed one iff
    max(|x - E| - 1/2, 0) >= max(|A - E| - 1/2, 0) (always, when no stratum is informative)."""
    A, E, V = S10.exact(tables)
    half = Fraction(1, 2)
    return V == 0 or max(abs(x - E) - half, 0) >= max(abs(A - E) - half, 0)


def csr(a, m, k, n):
    """The tables of every (trait, gene): a, m int [T, G, S], k, n int [T, S] -> (lo int32 [T, G], off int64
    [T G + 1], tab float64 [entries], A int64 [T, G]) in the layout of the device tables."""
    T, G, _S = a.shape
    lo, off, tab, A = np.zeros((T, G), np.int32), np.zeros(T * G + 1, np.int64), [], np.zeros((T, G), np.int64)
    for t in range(T):
        kt, nt = k[t].tolist(), n[t].tolist()
        for g in range(G):
            lo[t, g], row, A[t, g] = table(list(zip(a[t, g].tolist(), m[t, g].tolist(), kt, nt)))
            off[t * G + g + 1] = off[t * G + g] + len(row)
            tab.append(row)
    return lo, off, np.concatenate(tab), A


def observed(lo, off, tab, A):
    """Step 4: u_obs [T, G], every gene's own entry at x = A."""
    T, G = lo.shape
    return tab[off[:-1].reshape(T, G) + (A - lo)]


def permuted(lo, off, tab, t, a_perm):
    """u of trait t's genes under the pooled counts a_perm int [P, G] (each inside its gene's support)."""
    G = lo.shape[1]
    assert (a_perm >= lo[t][None]).all() and (a_perm - lo[t][None] < np.diff(off)[t * G:(t + 1) * G][None]).all()
    return tab[off[t * G:(t + 1) * G][None] + (a_perm - lo[t][None])]


def single_step(u_perm, u_obs):
    """Step 5: (minu [P], r_cmh_fwer [G]) of one trait from u_perm [P, G] and u_obs [G]."""
    minu = u_perm.min(axis=1)
    return minu, (minu[:, None] <= u_obs[None, :]).sum(axis=0)


def step_down(u_perm, u_obs):
    """Step 6 = S8 with p := u_obs and p_pi := u: order by (u_obs, gene index), successive minima from the back,
    raw counts, tie groups take the count of their first position, running maximum, back to gene order."""
    _P, G = u_perm.shape
    order = np.lexsort((np.arange(G), u_obs))
    us = u_obs[order]
    q = np.minimum.accumulate(u_perm[:, order][:, ::-1], axis=1)[:, ::-1]
    c = (q <= us[None, :]).sum(axis=0)
    first = np.r_[True, us[1:] != us[:-1]]
    tied = c[np.flatnonzero(first)][np.cumsum(first) - 1]
    r = np.empty(G, np.int64)
    r[order] = np.maximum.accumulate(tied)
    return r, q[:, 0]


def labelings_range(tables):
    """Brute force: the set of pooled counts a' over ALL within-stratum labelings (every placement of a stratum's k
    positives on its n valid isolates, m of which carry the gene) -- per stratum the reachable overlaps, summed."""
    from itertools import combinations
    reach = {0}
    for _a, m, k, n in tables:
        if n == 0:
            continue
        carriers = set(range(m))                          # the gene's isolates among the stratum's n valid ones
        own = {len(carriers & set(pos)) for pos in combinations(range(n), k)}
        reach = {r + o for r in reach for o in own}
    return reach

