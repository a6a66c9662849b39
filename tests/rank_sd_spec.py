"""Spec S18 in plain numpy: Westfall-Young step-down maxT over the rank statistics of the
quantitative traits.  A helper, not a test; written from the specification, independently of the kernels and of the
engine, on top of rank_wy_spec (S17), whose statistic it takes as it is.  One trait at a time."""
import numpy as np

import rank_wy_spec as wy
import ranksum_spec as rsp

PLANTED_SEED, PLANTED_P = 0x5EED5EED1818, 99


def order_of(s_obs):
    """Step 1: the genes descending by s_obs, ties by ascending gene index -> int64 [G]."""
    s_obs = np.asarray(s_obs, dtype=np.float64)
    return np.asarray(sorted(range(len(s_obs)), key=lambda g: (-s_obs[g], g)), dtype=np.int64)


def successive_maxima(D, cc, iv, order):
    """Step 2: u float64 [G, P], u[k, pi] = max over j >= k of s(order[j], D[order[j], pi]); the identity is 0.0."""
    s = wy.stats(np.asarray(D, dtype=np.int64)[order], cc, np.asarray(iv, dtype=np.float64)[order])
    return np.maximum(np.maximum.accumulate(s[::-1], axis=0)[::-1], 0.0)


def raw_counts(u, ss):
    """Step 3: c[k] = #{pi : u[k, pi] >= ss[k]}, doubles compared exactly -> int64 [G]."""
    return (u >= np.asarray(ss, dtype=np.float64)[:, None]).sum(axis=1)


def tail(c, ss, order):
    """Steps 4 and 5: every position of a group of equal ss takes the c of the group's first position, then the
    running maximum along the ranks, scattered to gene order -> r_sd int64 [G]."""
    c = np.asarray(c, dtype=np.int64).copy()
    for k in range(1, len(c)):
        if ss[k] == ss[k - 1]:
            c[k] = c[k - 1]
    r_sd = np.empty(len(c), dtype=np.int64)
    r_sd[order] = np.maximum.accumulate(c)
    return r_sd


def stepdown(D, cc, iv, s_obs, order=None):
    """S18 of one trait: D int [G, P], iv and s_obs float64 [G] -> dict(order, ss, u, c (by rank), r_sd (by gene)).
    ``order``: another order of the genes that is descending in s_obs (the result must not depend on it)."""
    order = order_of(s_obs) if order is None else np.asarray(order, dtype=np.int64)
    ss = np.asarray(s_obs, dtype=np.float64)[order]
    assert (ss[:-1] >= ss[1:]).all()
    u = successive_maxima(D, cc, iv, order)
    c = raw_counts(u, ss)
    return dict(order=order, ss=ss, u=u, c=c, r_sd=tail(c, ss, order))


def adjusted_p(r_sd, P):
    """Step 6."""
    return (np.asarray(r_sd, dtype=np.float64) + 1.0) / (P + 1.0)


def planted_driver(G=40, N=60, P=99, seed=18):
    """The fixed input on which the step-down count is strictly below the single-step one: gene 0 follows the values
    (a driver whose s_obs no permuted row reaches), gene 1 is a weaker copy of it, the others are noise.  Returns
    (genes uint8 [G, N], values float64 [N])."""
    rng = np.random.default_rng(seed)
    values = rng.permutation(N) * 0.5 - 3.0
    genes = (rng.random((G, N)) < 0.5).astype(np.uint8)
    genes[0] = values > np.median(values)
    genes[1] = genes[0]
    flip = rng.choice(N, N // 4, replace=False)
    genes[1, flip] ^= 1
    return genes, values


def planted_problem():
    """planted_driver() and everything the restatements make of it under S15's permutation law with the seed
    PLANTED_SEED: (genes, values, the S17 problem, D [G, P], stepdown(), r, r_fwer)."""
    genes, values = planted_driver()
    pr = wy.ranksum_problem(genes.astype(np.int64), values)
    rows = [rsp.perm_row(PLANTED_SEED, 0, pi, pr["valid"], pr["rc"]) for pi in range(PLANTED_P)]
    D = wy.permuted(genes.astype(np.int64), rows)
    out = stepdown(D, pr["cc"], pr["iv"], pr["s_obs"])
    mx = wy.maxs(D, pr["cc"], pr["iv"])
    return genes, values, pr, D, out, wy.r_count(D, pr["d"]), wy.r_fwer(mx, pr["s_obs"])
