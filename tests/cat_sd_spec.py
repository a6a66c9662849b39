"""Spec S23 in plain numpy: Westfall-Young step-down maxT over the statistics of the categorical
traits.  A helper, not a test; written from the specification, independently of the kernels and of the engine, on top
of cat_wy_spec (S22), whose statistics, comparison points and maxima it takes as they are.  One trait at a time: the
cells are the float64 [P, G] array of S22's statistic of every gene under every permuted code row (cat_wy_spec.stats /
chi2_cells for the chi-square test, gcmh_spec.q_many / cat_wy_spec.gcmh_cells for the generalized CMH one)."""
import numpy as np

import cat_wy_spec as ws
import categorical_spec as cs
import gcmh_spec as gs
from rank_sd_spec import tail                                # steps 4 and 5 are S18's, unchanged

PLANTED_SEED, PLANTED_P, PLANTED_DRIVER_SEED = 0x5EED5EED2323, 99, 23


def order_of(thr):
    """Step 1: the genes descending by thr, ties by ascending gene index -> int64 [G]."""
    thr = np.asarray(thr, dtype=np.float64)
    return np.asarray(sorted(range(len(thr)), key=lambda g: (-thr[g], g)), dtype=np.int64)


def successive_maxima(cells, order):
    """Step 2: u float64 [G, P], u[k, pi] = max over j >= k of cells[pi, order[j]]; the identity is 0.0."""
    s = np.asarray(cells, dtype=np.float64).T[order]
    return np.maximum(np.maximum.accumulate(s[::-1], axis=0)[::-1], 0.0)


def raw_counts(u, tt):
    """Step 3: c[k] = #{pi : u[k, pi] >= tt[k]}, doubles compared exactly -> int64 [G]."""
    return (u >= np.asarray(tt, dtype=np.float64)[:, None]).sum(axis=1)


def stepdown(cells, thr, order=None):
    """S23 of one trait: cells float64 [P, G], thr float64 [G] -> dict(order, tt, u, c (by rank), r_sd (by gene)).
    ``order``: another order of the genes that is descending in thr (the result must not depend on it)."""
    order = order_of(thr) if order is None else np.asarray(order, dtype=np.int64)
    tt = np.asarray(thr, dtype=np.float64)[order]
    assert (tt[:-1] >= tt[1:]).all()
    u = successive_maxima(cells, order)
    c = raw_counts(u, tt)
    return dict(order=order, tt=tt, u=u, c=c, r_sd=tail(c, tt, order))


def adjusted_p(r_sd, P):
    """Step 6."""
    return (np.asarray(r_sd, dtype=np.float64) + 1.0) / (P + 1.0)


def tables(genes, rows, K=cs.MAX_CLASSES):
    """a[.., g, k] of 0/1 genes [G, N] against code rows [.., N]: matrix products of 0/1 doubles, exact far past any
    count there is."""
    onehot = (np.asarray(rows)[..., None] == np.arange(1, K + 1)).astype(np.float64)
    prod = np.einsum("gn,...nk->...gk", np.asarray(genes, dtype=np.float64), onehot, optimize=True)
    return np.rint(prod).astype(np.int64)


def chi2_trait(genes, codes, rows):
    """The chi-square test of one trait by the vectorised restatement routes: dict(nk, a_obs, ivm, s_obs, thr [G],
    cells [P, G], r [G] -- S20's count, decided in integers)."""
    codes = np.asarray(codes)
    nk = cs.sizes(codes.tolist(), cs.MAX_CLASSES)
    a_obs, a_perm = tables(genes, codes), tables(genes, rows)
    ivm = np.array([ws.ivm_of(a.tolist(), nk) for a in a_obs])
    s_obs = ws.stats(a_obs, nk, ivm)
    w = cs.weights(nk)
    # sum a_k^2 w_k in int64 where it fits, else in Python integers
    dt = np.int64 if 8 * max(w) * int(a_obs.sum(axis=-1).max(initial=0)) ** 2 < 1 << 62 else object
    w = np.array(w, dtype=dt)
    r = ((a_perm.astype(dt) ** 2) @ w >= ((a_obs.astype(dt) ** 2) @ w)[None]).sum(axis=0).astype(np.int64)
    return dict(nk=nk, a_obs=a_obs, ivm=ivm, s_obs=s_obs, thr=ws.thr_of(s_obs),
                cells=ws.stats(a_perm, nk, ivm).reshape(len(rows), len(genes)), r=r.reshape(len(genes)))


def gcmh_trait(genes, codes, strata, S, rows):
    """The generalized CMH test of one trait by the vectorised routes: dict(form, df, s_obs = q, thr [G], cells
    [P, G], r [G] = #{Q >= thr})."""
    codes, strata, genes = np.asarray(codes), np.asarray(strata), np.asarray(genes, dtype=np.int64)
    nsk = gs.margins(codes.tolist(), strata.tolist(), S)
    member = ((strata[:, None] == np.arange(S)) & (codes[:, None] != 0)).astype(np.int64)
    E, V = gs.moments_many(genes @ member, nsk)
    form, df = gs.factor_many(E, V, max(gs.klast(nsk) - 1, 0))
    q = gs.q_many(tables(genes, codes), form)
    thr = q * gs.ONE_MINUS_TAU
    cells = gs.q_many(tables(genes, rows), form).reshape(len(rows), len(genes))
    return dict(form=form, df=df, s_obs=q, thr=thr, cells=cells, r=(cells >= thr[None]).sum(axis=0))


def planted_driver(G=40, N=60, K=3, seed=PLANTED_DRIVER_SEED):
    """The fixed input on which the step-down count is strictly below the single-step one: gene 0 is the indicator of
    class 1 (a driver whose statistic no permuted row reaches), gene 1 a copy with 30 % of the isolates flipped, the
    others are noise.  Returns (genes uint8 [G, N], codes int64 [N] in 1 .. K, strata int64 [N] of two lineages)."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(1, K + 1, N)
    strata = rng.integers(0, 2, N)
    genes = (rng.random((G, N)) < 0.5).astype(np.uint8)
    genes[0] = codes == 1
    genes[1] = genes[0]
    genes[1, rng.choice(N, (3 * N) // 10, replace=False)] ^= 1
    return genes, codes, strata


def planted_problem(test):
    """planted_driver() and what the restatements make of it under the project's own permutation law with the seed
    PLANTED_SEED (``test``: "chi2" -- S15's shuffle over the labelled isolates -- or "gcmh" -- S16's shuffle within the
    strata): (genes, codes, strata, the trait's dict, stepdown(), r_fwer)."""
    genes, codes, strata = planted_driver()
    if test == "chi2":
        rows = np.array([cs.perm_row(PLANTED_SEED, 0, pi, codes.tolist()) for pi in range(PLANTED_P)])
        tr = chi2_trait(genes, codes, rows)
    else:
        rows = np.array([gs.perm_row(PLANTED_SEED, 0, pi, codes.tolist(), strata.tolist(), 2)
                         for pi in range(PLANTED_P)])
        tr = gcmh_trait(genes, codes, strata, 2, rows)
    out = stepdown(tr["cells"], tr["thr"])
    return genes, codes, strata, tr, out, ws.r_fwer(ws.maxs(tr["cells"]), tr["thr"])
